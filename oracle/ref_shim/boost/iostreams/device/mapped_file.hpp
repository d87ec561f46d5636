/* Stand-in for boost's read-only mapped file: the whole file read into memory. */
#ifndef MUMS_REF_SHIM_BOOST_MAPPED_FILE_HPP
#define MUMS_REF_SHIM_BOOST_MAPPED_FILE_HPP
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
namespace boost { namespace iostreams {
class mapped_file_source {
public:
	typedef size_t size_type;
	mapped_file_source() : opened(false) {}
	explicit mapped_file_source(const std::string& path) : opened(false) { open(path); }
	void open(const std::string& path) {
		std::ifstream in(path.c_str(), std::ios::binary);
		opened = in.is_open();
		if (opened)
			bytes.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
	}
	bool is_open() const { return opened; }
	void close() { bytes.clear(); opened = false; }
	size_type size() const { return bytes.size(); }
	const char* data() const { return bytes.empty() ? 0 : &bytes[0]; }
private:
	std::vector<char> bytes;
	bool opened;
};
} }
#endif
