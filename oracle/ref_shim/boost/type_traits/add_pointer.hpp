#ifndef MUMS_REF_SHIM_BOOST_ADD_POINTER_HPP
#define MUMS_REF_SHIM_BOOST_ADD_POINTER_HPP
#include <type_traits>
namespace boost { using std::add_pointer; }
#endif
