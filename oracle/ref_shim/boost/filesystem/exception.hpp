#ifndef MUMS_REF_SHIM_BOOST_FILESYSTEM_exception_HPP
#define MUMS_REF_SHIM_BOOST_FILESYSTEM_exception_HPP
#include "boost/filesystem.hpp"
#endif
