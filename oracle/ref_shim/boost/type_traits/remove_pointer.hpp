#ifndef MUMS_REF_SHIM_BOOST_REMOVE_POINTER_HPP
#define MUMS_REF_SHIM_BOOST_REMOVE_POINTER_HPP
#include <type_traits>
namespace boost { using std::remove_pointer; }
#endif
