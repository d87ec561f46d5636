/* Stand-in for MUSCLE's thread-local holder: one T per OpenMP thread. */
#ifndef MUMS_REF_SHIM_THREADSTORAGE_H
#define MUMS_REF_SHIM_THREADSTORAGE_H
#include <cstddef>
#include <vector>
#ifdef _OPENMP
#include <omp.h>
#endif

template <class T>
class TLS {
public:
	TLS() : slots(slot_count()) {}
	explicit TLS(const T& v) : slots(slot_count(), v) {}
	T& get() { return slots[slot()]; }
	const T& get() const { return slots[slot()]; }
private:
	static size_t slot_count() {
#ifdef _OPENMP
		int n = omp_get_max_threads();
		return n < 64 ? 64 : (size_t)n;
#else
		return 1;
#endif
	}
	static size_t slot() {
#ifdef _OPENMP
		return (size_t)omp_get_thread_num();
#else
		return 0;
#endif
	}
	std::vector<T> slots;
};
#endif
