/* Stand-in for boost::object_pool: construct and destroy single objects. */
#ifndef MUMS_REF_SHIM_BOOST_OBJECT_POOL_HPP
#define MUMS_REF_SHIM_BOOST_OBJECT_POOL_HPP
#include <cstddef>
namespace boost {
template <class T>
class object_pool {
public:
	explicit object_pool(size_t = 32) {}
	T* construct() { return new T(); }
	template <class A> T* construct(const A& a) { return new T(a); }
	void destroy(T* p) { delete p; }
};
}
#endif
