/* Shadows the reference header of the same name: a sequence read whole from a
   raw file into memory. */
#ifndef MUMS_REF_SHIM_GNRAWSEQUENCE_H
#define MUMS_REF_SHIM_GNRAWSEQUENCE_H
#include "libGenome/gnSequence.h"
#include <fstream>
#include <iterator>
namespace genome {
class gnRAWSequence : public gnSequence {
public:
	gnRAWSequence() {}
	explicit gnRAWSequence(const std::string& filename) {
		std::ifstream in(filename.c_str(), std::ios::binary);
		if (!in.is_open())
			Throw_gnEx(FileNotOpened());
		m_seq.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
		m_spec.SetName(filename);
	}
	virtual gnRAWSequence* Clone() const { return new gnRAWSequence(*this); }
};
}
#endif
