/* Stand-in for the autoconf header the libMems sources include first.
   Nothing in the units the reference driver links depends on a setting. */
#ifndef MUMS_REF_SHIM_CONFIG_H
#define MUMS_REF_SHIM_CONFIG_H
#endif
