/* Stand-in for libGenome's raw sequence file writer. */
#ifndef MUMS_REF_SHIM_GNRAWSOURCE_H
#define MUMS_REF_SHIM_GNRAWSOURCE_H
#include "libGenome/gnSequence.h"
#include <fstream>
namespace genome {
class gnRAWSource {
public:
	static boolean Write(gnSequence& seq, const std::string& filename) {
		std::ofstream out(filename.c_str(), std::ios::binary);
		if (!out.is_open())
			return false;
		out << seq.ToString();
		return true;
	}
};
}
#endif
