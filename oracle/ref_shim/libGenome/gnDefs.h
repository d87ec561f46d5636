/* Stand-in for libGenome's basic definitions: only what the libMems match
   finder needs, written from how libMems uses the names. */
#ifndef MUMS_REF_SHIM_GNDEFS_H
#define MUMS_REF_SHIM_GNDEFS_H

#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

typedef uint8_t uint8;
typedef int8_t int8;
typedef uint16_t uint16;
typedef int16_t int16;
typedef uint32_t uint32;
typedef int32_t int32;
typedef uint64_t uint64;
typedef int64_t int64;
typedef int8_t sint8;
typedef int16_t sint16;
typedef int32_t sint32;
typedef int64_t sint64;
typedef unsigned int uint;
typedef float float32;
typedef double float64;
typedef bool boolean;

typedef uint64 gnSeqI;
typedef char gnSeqC;

#ifndef UINT8_MAX
#define UINT8_MAX 255
#endif
#ifndef UINT32_MAX
#define UINT32_MAX 4294967295U
#endif

#define GNSEQI_END (std::numeric_limits<gnSeqI>::max())
#define GNSEQI_ERROR (GNSEQI_END - 1)
#define GNSEQC_NULL 0
#define ALL_CONTIGS UINT32_MAX
#define GNSEQI_BEGIN 0
#define GNSEQC_MAX 127
#define GNSEQC_MIN 0

#define GNOME_DLL_API

namespace genome {

template <class T>
inline T absolut(const T& v) { return v < 0 ? -v : v; }

/* Heap buffer that frees itself; libMems reads and writes it through .data. */
template <class T>
class Array {
public:
	explicit Array(uint64 n) : data(new T[n]()), count(n) {}
	~Array() { delete[] data; }
	T* data;
	uint64 count;
private:
	Array(const Array&);
	Array& operator=(const Array&);
};

}  // namespace genome

#endif
