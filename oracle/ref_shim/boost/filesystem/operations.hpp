#ifndef MUMS_REF_SHIM_BOOST_FILESYSTEM_operations_HPP
#define MUMS_REF_SHIM_BOOST_FILESYSTEM_operations_HPP
#include "boost/filesystem.hpp"
#endif
