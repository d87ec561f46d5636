/* Stand-in for libGenome's clonable base class. */
#ifndef MUMS_REF_SHIM_GNCLONE_H
#define MUMS_REF_SHIM_GNCLONE_H
#include "libGenome/gnDefs.h"
namespace genome {
class gnClone {
public:
	virtual ~gnClone() {}
	virtual gnClone* Clone() const = 0;
};
}
#endif
