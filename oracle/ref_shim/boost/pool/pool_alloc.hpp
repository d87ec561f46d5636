/* Stand-in for boost's pool allocators on top of the standard allocator. */
#ifndef MUMS_REF_SHIM_BOOST_POOL_ALLOC_HPP
#define MUMS_REF_SHIM_BOOST_POOL_ALLOC_HPP
#include <memory>
namespace boost {
template <class T>
class pool_allocator : public std::allocator<T> {
public:
	template <class U> struct rebind { typedef pool_allocator<U> other; };
	pool_allocator() {}
	template <class U> pool_allocator(const pool_allocator<U>&) {}
};
template <class T>
class fast_pool_allocator : public std::allocator<T> {
public:
	template <class U> struct rebind { typedef fast_pool_allocator<U> other; };
	fast_pool_allocator() {}
	template <class U> fast_pool_allocator(const fast_pool_allocator<U>&) {}
	static T* allocate() { return static_cast<T*>(::operator new(sizeof(T))); }
	static T* allocate(size_t n) { return static_cast<T*>(::operator new(n * sizeof(T))); }
	static void deallocate(T* p) { ::operator delete(p); }
	static void deallocate(T* p, size_t) { ::operator delete(p); }
};
}
#endif
