/* Stand-in for the few boost::filesystem calls libMems makes. */
#ifndef MUMS_REF_SHIM_BOOST_FILESYSTEM_HPP
#define MUMS_REF_SHIM_BOOST_FILESYSTEM_HPP
#include <stdio.h>
#include <sys/stat.h>
#include <stdexcept>
#include <string>
namespace boost { namespace filesystem {
class path {
public:
	path() {}
	path(const char* s) : p(s) {}
	path(const std::string& s) : p(s) {}
	const std::string& string() const { return p; }
	const char* c_str() const { return p.c_str(); }
private:
	std::string p;
};
class filesystem_error : public std::runtime_error {
public:
	explicit filesystem_error(const std::string& m) : std::runtime_error(m) {}
};
inline bool exists(const path& p) { struct stat st; return stat(p.c_str(), &st) == 0; }
inline bool remove(const path& p) { return ::remove(p.c_str()) == 0; }
} }
#endif
