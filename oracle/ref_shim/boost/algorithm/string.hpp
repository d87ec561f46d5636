/* Stand-in for boost::algorithm::replace_all. */
#ifndef MUMS_REF_SHIM_BOOST_ALGORITHM_STRING_HPP
#define MUMS_REF_SHIM_BOOST_ALGORITHM_STRING_HPP
#include <string>
namespace boost { namespace algorithm {
inline void replace_all(std::string& s, const std::string& from, const std::string& to) {
	if (from.empty())
		return;
	for (size_t at = s.find(from); at != std::string::npos; at = s.find(from, at + to.size()))
		s.replace(at, from.size(), to);
}
} using algorithm::replace_all; }
#endif
