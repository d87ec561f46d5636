/* Stand-in for boost::dynamic_bitset with the operations libMems calls. */
#ifndef MUMS_REF_SHIM_BOOST_DYNAMIC_BITSET_HPP
#define MUMS_REF_SHIM_BOOST_DYNAMIC_BITSET_HPP
#include <cstddef>
#include <memory>
#include <vector>
namespace boost {
template <class Block = unsigned long, class Alloc = std::allocator<Block> >
class dynamic_bitset {
public:
	typedef size_t size_type;
	static const size_type npos = (size_type)-1;
	class reference {
	public:
		reference(std::vector<unsigned char>& b, size_type i) : bits(b), pos(i) {}
		operator bool() const { return bits[pos] != 0; }
		reference& operator=(bool v) { bits[pos] = v; return *this; }
		reference& operator=(const reference& r) { bits[pos] = (bool)r; return *this; }
		reference& flip() { bits[pos] = !bits[pos]; return *this; }
		bool operator~() const { return !bits[pos]; }
	private:
		std::vector<unsigned char>& bits;
		size_type pos;
	};
	dynamic_bitset() {}
	explicit dynamic_bitset(size_type n, unsigned long value = 0) : bits(n, 0) {
		for (size_type i = 0; i < n && i < 8 * sizeof value; i++)
			bits[i] = (value >> i) & 1;
	}
	size_type size() const { return bits.size(); }
	bool empty() const { return bits.empty(); }
	void resize(size_type n, bool v = false) { bits.resize(n, v); }
	void clear() { bits.clear(); }
	void push_back(bool v) { bits.push_back(v); }
	bool test(size_type i) const { return bits[i] != 0; }
	bool operator[](size_type i) const { return bits[i] != 0; }
	reference operator[](size_type i) { return reference(bits, i); }
	dynamic_bitset& set() { bits.assign(bits.size(), 1); return *this; }
	dynamic_bitset& set(size_type i, bool v = true) { bits[i] = v; return *this; }
	dynamic_bitset& reset() { bits.assign(bits.size(), 0); return *this; }
	dynamic_bitset& reset(size_type i) { bits[i] = 0; return *this; }
	dynamic_bitset& flip() { for (size_type i = 0; i < bits.size(); i++) bits[i] = !bits[i]; return *this; }
	dynamic_bitset& flip(size_type i) { bits[i] = !bits[i]; return *this; }
	size_type count() const { size_type c = 0; for (size_type i = 0; i < bits.size(); i++) c += bits[i]; return c; }
	bool any() const { return count() != 0; }
	bool none() const { return count() == 0; }
	size_type find_first() const { return find_from(0); }
	size_type find_next(size_type i) const { return find_from(i + 1); }
	dynamic_bitset& operator&=(const dynamic_bitset& o) { for (size_type i = 0; i < bits.size(); i++) bits[i] &= o.bits[i]; return *this; }
	dynamic_bitset& operator|=(const dynamic_bitset& o) { for (size_type i = 0; i < bits.size(); i++) bits[i] |= o.bits[i]; return *this; }
	dynamic_bitset& operator^=(const dynamic_bitset& o) { for (size_type i = 0; i < bits.size(); i++) bits[i] ^= o.bits[i]; return *this; }
	dynamic_bitset operator~() const { dynamic_bitset r(*this); r.flip(); return r; }
	bool operator==(const dynamic_bitset& o) const { return bits == o.bits; }
	bool operator!=(const dynamic_bitset& o) const { return bits != o.bits; }
	void swap(dynamic_bitset& o) { bits.swap(o.bits); }
private:
	size_type find_from(size_type i) const {
		for (; i < bits.size(); i++)
			if (bits[i])
				return i;
		return npos;
	}
	std::vector<unsigned char> bits;
};
template <class B, class A>
inline dynamic_bitset<B, A> operator&(dynamic_bitset<B, A> a, const dynamic_bitset<B, A>& b) { return a &= b; }
template <class B, class A>
inline dynamic_bitset<B, A> operator|(dynamic_bitset<B, A> a, const dynamic_bitset<B, A>& b) { return a |= b; }
template <class B, class A>
inline dynamic_bitset<B, A> operator^(dynamic_bitset<B, A> a, const dynamic_bitset<B, A>& b) { return a ^= b; }
}
#endif
