/* Stand-in for libGenome's message helpers. */
#ifndef MUMS_REF_SHIM_GNDEBUG_H
#define MUMS_REF_SHIM_GNDEBUG_H
#include "libGenome/gnDefs.h"
namespace genome {
inline void DebugMsg(const std::string& m) { std::cerr << m; }
inline void ErrorMsg(const std::string& m) { std::cerr << m; }
}
#endif
