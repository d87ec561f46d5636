/* Stand-in: the match finder includes the filter header but uses none of it. */
#ifndef MUMS_REF_SHIM_GNFILTER_H
#define MUMS_REF_SHIM_GNFILTER_H
#include "libGenome/gnDefs.h"
#endif
