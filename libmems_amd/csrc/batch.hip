// batch.hip -- many small MemHash::FindMatches in one device pass (mums_find_batch).
//
// B independent problems of G sequences each.  Problem p's MatchList must be what
// MemHash::FindMatches (MemHash.cpp:109-115) returns for p alone, so everything that compares
// entries runs in p's own coordinates:
//   keys    one thread per seed-mer of the whole batch (compact index i = mbase[p * G + g] + position;
//           only windows inside their own sequence exist): key2 = p << (2w+1) | ckey, read from ASCII
//   sort    radix_sort<u64> on 2w+1 + ceil(log2 B) bits: groups are (p, masked key) runs
//   replay  one lane per problem walks its run of the sorted stream in key order: MemHash::
//           EnumerateMatches (MemHash.cpp:139-162, default tolerances), HashMatch (:167-187,
//           MaskedMemHash.cpp:38-63), AddHashEntry (:209-251: lower_bound over the bucket vector with
//           MheCompare, MatchHashEntry.h:121-143) and ExtendMatch (MatchFinder.h:218-374) as the
//           reference runs them, on local starts.  The problem's table is one array of (bucket, entry)
//           sorted by bucket, each bucket's part in vector order: bucket-major is GetMatchList order.
//   emit    one workgroup per problem copies its entries to its rows of the batch's MatchList.
// A problem the lane cannot finish (a masked-key group above MER_REPEAT_LIMIT, entry pool full) is
// flagged and left to the caller, which runs it through the single-problem pipeline.
#include <hip/hip_runtime.h>

#include "mums_internal.h"
#include "seed_device.h"

namespace mums {

namespace {

constexpr int kBatchBlock = 64;   // replay: lanes (= problems) per workgroup

// BasicDNATable (SortedMerList.cpp:29-47)
__device__ __forceinline__ uint64_t batch_dna2(uint32_t c) {
    const uint32_t lc = c | 0x20u;
    const uint32_t one = (lc == 'c') | (lc == 'b') | (lc == 'y');
    const uint32_t two = (lc == 'g') | (lc == 's') | (lc == 'k');
    const uint32_t three = (lc == 't');
    return one | (two << 1) | (three * 3u);
}

// first byte offset holding '-' (atomicMin), ~0 when none
__global__ void batch_gap_kernel(const char* __restrict__ a, uint64_t lo, uint64_t hi,
                                 unsigned long long* __restrict__ first) {
    const uint64_t i0 = lo + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (i0 >= hi) return;
    const uint64_t i1 = i0 + 16 < hi ? i0 + 16 : hi;
    for (uint64_t i = i0; i < i1; ++i)
        if (a[i] == '-') {
            atomicMin(first, (unsigned long long)i);
            return;
        }
}

// seg = the sequence holding compact seed-mer index i: the largest s with mbase[s] <= i
__device__ __forceinline__ uint32_t batch_seg_of(const uint32_t* __restrict__ mbase, uint32_t nseg, uint32_t i) {
    uint32_t lo = 0, hi = nseg;   // mbase[lo] <= i < mbase[hi] (mbase[nseg] = N > i)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (mbase[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void batch_keys_kernel(const char* __restrict__ ascii, const uint64_t* __restrict__ aoff,
                                  const uint32_t* __restrict__ mbase, uint32_t nseg, uint32_t G, uint32_t N,
                                  SeedSpec ss, int kbits, uint64_t* __restrict__ keys) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    const uint32_t i = (uint32_t)t;
    const uint32_t seg = batch_seg_of(mbase, nseg, i);
    const char* src = ascii + aoff[seg] + (i - mbase[seg]);   // the L-window lies inside the sequence
    uint64_t mer = 0;
    for (int k = 0; k < ss.L; ++k) mer |= batch_dna2((unsigned char)src[k]) << (62 - 2 * k);
    const uint64_t p = seg / G;
    keys[i] = (p << kbits) | ckey_from_mer(mer, ss);
}

// MatchHashEntry (MatchHashEntry.h:30-103): starts padded with NO_MATCH up to MG (neutral in
// every comparison below)
template <int MG>
struct Mhe {
    int64_t len, off, mer;
    int64_t s[MG];
};

// constant-trip loops over the starts: unrolled (registers) up to 8 sequences, scratch arrays above
template <int MG>
constexpr int kMgUnroll = MG <= 8 ? MG : 1;
#define MG_UNROLL _Pragma("unroll kMgUnroll<MG>")

template <int MG>
__device__ __forceinline__ int mhe_first(const Mhe<MG>& m) {   // FirstStart, HybridAbstractMatch.h:121-129
    int f = 0x7fffffff;
    MG_UNROLL
    for (int i = MG - 1; i >= 0; --i)
        if (m.s[i] != 0) f = i;
    return f;
}

// Contains: MatchHashEntry.cpp:164-200 (does a contain b); fb = FirstStart(b)
template <int MG>
__device__ __forceinline__ bool mhe_contains(const Mhe<MG>& a, const Mhe<MG>& b, int fb) {
    if (a.off != b.off) return false;
    int64_t as = 0, bs = 0;
    MG_UNROLL
    for (int i = 0; i < MG; ++i)
        if (i == fb) { as = a.s[i]; bs = b.s[i]; }
    const int64_t diff = bs - as;
    if (as == 0) return false;
    if (diff < 0 || a.len < b.len + diff) return false;
    const int64_t diff_rc = b.len - a.len + diff;
    bool ok = true;
    MG_UNROLL
    for (int i = 0; i < MG; ++i) {
        if (i <= fb) continue;
        const int64_t di = b.s[i] - a.s[i];
        if (b.s[i] == 0 && a.s[i] == 0) continue;
        if (b.s[i] < 0 && diff_rc == di) continue;
        if (diff != di) ok = false;
    }
    return ok;
}

// MheCompare: MatchHashEntry.h:121-143, strict_start_lessthan_ptr: MatchHashEntry.cpp:48-69
template <int MG>
__device__ __forceinline__ bool mhe_less(const Mhe<MG>& a, const Mhe<MG>& b) {
    const int fa = mhe_first(a), fb = mhe_first(b);
    if (fa > fb) return true;
    if (fa < fb) return false;
    int pres = 0;   // the first genome present in one only decides: 1 = a lacks it, 2 = b lacks it
    MG_UNROLL
    for (int i = 0; i < MG; ++i) {
        if (pres == 0 && a.s[i] == 0 && b.s[i] != 0) pres = 1;
        if (pres == 0 && a.s[i] != 0 && b.s[i] == 0) pres = 2;
    }
    if (pres) return pres == 1;
    if (mhe_contains(a, b, fb) || mhe_contains(b, a, fa)) return false;
    int dec = 0;
    MG_UNROLL
    for (int i = 0; i < MG; ++i) {
        int64_t as = a.s[i], bs = b.s[i];
        if (as < 0) as = -as + a.len - a.mer;
        if (bs < 0) bs = -bs + b.len - b.mer;
        if (dec == 0 && as != bs) dec = as < bs ? 1 : 2;
    }
    return dec == 1;
}

template <int MG>
__device__ __forceinline__ void mhe_load(Mhe<MG>& e, const int64_t* __restrict__ row, int G) {
    e.len = row[0];
    e.off = row[1];
    e.mer = 0;   // stored copies: operator=, MatchHashEntry.cpp:118-126
    MG_UNROLL
    for (int i = 0; i < MG; ++i) e.s[i] = i < G ? row[2 + i] : 0;
}

// std::lower_bound over the bucket vector ord[lo, hi) (libstdc++ __lower_bound)
template <int MG>
__device__ __forceinline__ uint32_t mhe_lower_bound(const uint64_t* __restrict__ ord, uint32_t lo, uint32_t hi,
                                                    const int64_t* __restrict__ pool, int G, const Mhe<MG>& val) {
    uint32_t first = lo, len = hi - lo;
    Mhe<MG> e;
    while (len > 0) {
        const uint32_t half = len >> 1, mid = first + half;
        mhe_load(e, pool + (uint64_t)(uint32_t)ord[mid] * (uint64_t)(G + 2), G);
        if (mhe_less(e, val)) { first = mid + 1; len = len - half - 1; }
        else len = half;
    }
    return first;
}

struct BatchSeg {   // one problem's sequences
    const uint32_t* mb;   // compact index of position 0 of sequence g (G + 1 entries)
    const uint64_t* n;    // sequence lengths
};

// the oriented seed ExtendMatch tests (MatchFinder.h:265-293): masked key and strand of genome g's
// seed at the match's moving end
template <int MG>
__device__ __forceinline__ bool batch_seed_at(const Mhe<MG>& m, int g, int64_t sg, const BatchSeg& q, int L,
                                              const uint64_t* __restrict__ keys, uint64_t* key, uint32_t* par) {
    int64_t mt = sg;
    if (mt < 0) mt = -mt + m.len - L;
    const uint64_t idx = (uint64_t)(mt - 1), mg = (uint64_t)(q.mb[g + 1] - q.mb[g]);
    if (idx >= mg) return false;   // never taken: maxlen keeps the seed inside the sequence
    const uint64_t k = keys[(uint64_t)q.mb[g] + idx];
    *par = sg < 0 ? (uint32_t)(k & 1) : (uint32_t)((k & 1) ^ 1);
    *key = k >> 1;
    return true;
}

// ExtendMatch: MatchFinder.h:218-374 (linear sequences); returns false on an index outside a
// sequence (a flaw in this restatement, never an input property: the problem is then flagged)
template <int MG>
__device__ bool batch_extend(Mhe<MG>& m, int G, const BatchSeg& q, int L, const uint64_t* __restrict__ keys) {
    uint64_t pm = 0;
    int g0 = -1;
    for (int g = G - 1; g >= 0; --g)
        if (m.s[g] != 0) { pm |= 1ull << g; g0 = g; }
    int jump = L;
    bool extend_again = false;
    bool fine = true;
    for (int dir = 0; dir < 4; ++dir) {
        int64_t maxlen = dir < 2 ? INT64_MAX : (int64_t)L;
        MG_UNROLL
        for (int g = 0; g < MG; ++g) {
            if (!((pm >> g) & 1)) continue;
            if (m.s[g] < 0) {
                const int64_t rc_len = (int64_t)q.n[g] - m.len + m.s[g] + 1;
                if (rc_len < maxlen) maxlen = rc_len;
            } else if (m.s[g] - 1 < maxlen) {
                maxlen = m.s[g] - 1;
            }
        }
        bool mis = false, moved = false;
        uint64_t extend_limit = 0, extend_attempts = 0;
        while (maxlen - jump >= 0) {
            m.len += jump;
            maxlen -= jump;
            moved = true;
            MG_UNROLL
            for (int g = 0; g < MG; ++g)
                if (((pm >> g) & 1) && m.s[g] > 0) {
                    m.s[g] -= jump;
                    if (m.s[g] <= 0) m.s[g] += (int64_t)q.n[g];
                }
            uint64_t k0 = 0;
            uint32_t p0 = 0;
            mis = false;
            MG_UNROLL
            for (int g = 0; g < MG; ++g) {
                if (!((pm >> g) & 1)) continue;
                uint64_t kg = 0;
                uint32_t pg = 0;
                if (!batch_seed_at(m, g, m.s[g], q, L, keys, &kg, &pg)) { fine = false; mis = true; }
                if (g == g0) { k0 = kg; p0 = pg; }
                else if (kg != k0 || pg != p0) mis = true;
            }
            if (mis && dir < 2) maxlen = 0;
            extend_attempts += (uint64_t)jump;
            if (!mis) extend_limit = extend_attempts;
            if (dir > 1 && extend_attempts == (uint64_t)L) break;
        }
        if (moved && mis) {
            m.len -= jump;
            MG_UNROLL
            for (int g = 0; g < MG; ++g)
                if (((pm >> g) & 1) && m.s[g] >= 0) m.s[g] += jump;
        }
        if (dir > 1 && extend_attempts > 0) {
            if (extend_limit > 0) extend_again = true;
            int64_t unmatched = (int64_t)(extend_attempts - extend_limit);
            if (moved && mis) unmatched -= jump;
            m.len -= unmatched;
            MG_UNROLL
            for (int g = 0; g < MG; ++g)
                if (((pm >> g) & 1) && m.s[g] > 0) {
                    m.s[g] += unmatched;
                    if (m.s[g] > (int64_t)q.n[g]) m.s[g] -= (int64_t)q.n[g];
                }
        }
        MG_UNROLL
        for (int g = 0; g < MG; ++g) m.s[g] = -m.s[g];   // Invert, HybridAbstractMatch.h:206-213
        if (dir >= 1) jump = 1;
        if (dir == 3 && extend_again) { dir = -1; jump = L; extend_again = false; }
    }
    return fine;
}

struct BatchReplayArgs {
    const uint64_t* sk;       // sorted key2
    const uint32_t* sv;       // sorted compact indices
    const uint64_t* keys;     // key2 by compact index
    const uint32_t* mbase;    // B * G + 1
    const uint64_t* nlen;     // B * G sequence lengths
    const uint32_t* order;    // lane -> problem (problems of similar size share a wave)
    uint64_t* ord;            // (bucket << 32 | entry) per problem at mbase[p * G] / 2
    int64_t* pool;            // entries {len, offset, starts}
    uint32_t pool_cap;
    uint32_t* pool_n;
    uint32_t* cnt;            // per problem: entries
    uint32_t* probes;         // AddHashEntry calls
    uint32_t* coll;           // MemCollisionCount
    uint32_t* flag;           // 1 group above MER_REPEAT_LIMIT, 2 pool full, 4 internal
    uint32_t B, G;
    int L, kbits;
    uint32_t table_size;
    int masked;
    uint64_t seq_mask;
    const uint32_t* ord_base;   // CARRY: problem p's slice of ord and its capacity
    const uint32_t* ord_cap;
};

// CARRY (mums_anchor_batch): one round of a seed family.  The lane goes on from the
// table the rounds before left in its slice (MemHash::ClearSequences keeps the table,
// ProgressiveAligner.cpp:619-653): AddHashEntry's search below already is the keep rule, the stored
// entries compare with mer = 0 and the probes with this round's L.
template <int MG, bool CARRY>
__device__ __forceinline__ void batch_replay_lane(const BatchReplayArgs& a) {
    const uint32_t t = blockIdx.x * kBatchBlock + threadIdx.x;
    if (t >= a.B) return;
    const uint32_t p = a.order[t];
    const int G = (int)a.G;
    const uint32_t* mb = a.mbase + (uint64_t)p * a.G;
    const BatchSeg q{mb, a.nlen + (uint64_t)p * a.G};
    const uint32_t r0 = mb[0], r1 = mb[G];
    uint64_t* ord = a.ord + (CARRY ? a.ord_base[p] : (r0 >> 1));
    const uint32_t ord_cap = CARRY ? a.ord_cap[p] : (r1 - r0) >> 1;   // one entry needs a probe, a probe two records
    const uint64_t stride = (uint64_t)(G + 2);
    const int64_t T = (int64_t)a.table_size;
    uint32_t n = 0, probes = 0, coll = 0, flag = 0;
    if (CARRY) {
        n = a.cnt[p];
        probes = a.probes[p];
        coll = a.coll[p];
        flag = a.flag[p];
    }
    uint32_t c_bi = ~0u, c_lo = 0, c_hi = 0;   // the last probe's bucket (< 2^31) and its vector, until an insert

    uint32_t i = r0;
    while (i < r1 && !flag) {
        // one (p, masked key) group [i, j)
        const uint64_t gk = a.sk[i] >> 1;
        uint32_t j = i + 1;
        while (j < r1 && (a.sk[j] >> 1) == gk) ++j;
        const uint32_t gs = j - i;
        if (gs > (uint32_t)kRepeatLimit) { flag = 1; break; }   // SearchRange would restart (MatchFinder.cpp:253-277)
        if (gs < 2) { i = j; continue; }
        // MemHash::EnumerateMatches, repeat tolerance 0 / enumeration tolerance 1: a genome twice drops the group
        Mhe<MG> m;
        MG_UNROLL
        for (int g = 0; g < MG; ++g) m.s[g] = 0;
        uint64_t seen = 0, parbits = 0;
        bool dup = false;
        for (uint32_t k = i; k < j; ++k) {
            const uint32_t idx = a.sv[k];
            int g = 0;
            for (int h = 1; h < G; ++h) g += idx >= mb[h] ? 1 : 0;
            if ((seen >> g) & 1) { dup = true; break; }
            seen |= 1ull << g;
            parbits |= (a.sk[k] & 1ull) << g;
            const int64_t s1 = (int64_t)(idx - mb[g]) + 1;
            MG_UNROLL
            for (int h = 0; h < MG; ++h)
                if (h == g) m.s[h] = s1;
        }
        i = j;
        if (dup) continue;
        // HashMatch (MemHash.cpp:167-187) + SetDirection (:189-203)
        const int ref = __builtin_ctzll(seen);
        const uint32_t ref_forward = (uint32_t)((parbits >> ref) & 1) ^ 1u;
        int mult = 0;
        uint64_t match_number = 0;
        MG_UNROLL
        for (int g = 0; g < MG; ++g) {
            if (g >= G) continue;
            match_number <<= 1;
            if (m.s[g] != 0) {
                match_number |= 1;
                ++mult;
                if (g > ref && ref_forward == (uint32_t)((parbits >> g) & 1)) m.s[g] = -m.s[g];
            }
        }
        m.len = a.L;
        m.mer = a.L;
        {   // CalculateOffset: MatchHashEntry.cpp:141-160
            int64_t off = 0, sr = 0;
            MG_UNROLL
            for (int g = 0; g < MG; ++g) {
                if (g == ref) sr = m.s[g];
                if (g > ref && m.s[g] != 0) {
                    int64_t d = m.s[g] - sr;
                    if (m.s[g] < 0) d -= m.len;
                    off += d;
                }
            }
            m.off = off;
        }
        if (a.masked ? !(a.seq_mask == 0 || match_number == a.seq_mask) : mult < 2) continue;
        // AddHashEntry: MemHash.cpp:209-251
        ++probes;
        const uint32_t bi = (uint32_t)(((m.off % T) + T) % T);
        uint32_t lo = c_lo, hi = c_hi;   // the bucket's vector = ord[lo, hi)
        if (bi != c_bi) {
            uint32_t x = 0, y = n;
            while (x < y) {
                const uint32_t mid = (x + y) >> 1;
                if ((uint32_t)(ord[mid] >> 32) < bi) x = mid + 1;
                else y = mid;
            }
            lo = x;
            y = n;
            while (x < y) {
                const uint32_t mid = (x + y) >> 1;
                if ((uint32_t)(ord[mid] >> 32) <= bi) x = mid + 1;
                else y = mid;
            }
            hi = x;
            c_bi = bi;
            c_lo = lo;
            c_hi = hi;
        }
        const uint32_t it = mhe_lower_bound<MG>(ord, lo, hi, a.pool, G, m);
        if (it != hi) {
            Mhe<MG> e;
            mhe_load(e, a.pool + (uint64_t)(uint32_t)ord[it] * stride, G);
            if (!mhe_less(e, m) && !mhe_less(m, e)) { ++coll; continue; }
        }
        if (!batch_extend<MG>(m, G, q, a.L, a.keys)) { flag = 4; break; }
        m.mer = 0;
        const uint32_t id = atomicAdd(a.pool_n, 1u);
        if (id >= a.pool_cap || n >= ord_cap) { flag = 2; break; }
        int64_t* row = a.pool + (uint64_t)id * stride;
        row[0] = m.len;
        row[1] = m.off;
        MG_UNROLL
        for (int g = 0; g < MG; ++g)
            if (g < G) row[2 + g] = m.s[g];
        const uint32_t ins = mhe_lower_bound<MG>(ord, lo, hi, a.pool, G, m);
        for (uint32_t k = n; k > ins; --k) ord[k] = ord[k - 1];
        ord[ins] = ((uint64_t)bi << 32) | id;
        ++n;
        c_bi = ~0u;
    }
    a.cnt[p] = flag ? 0u : n;
    a.probes[p] = probes;
    a.coll[p] = coll;
    a.flag[p] = flag;
}

template <int MG>
__global__ __launch_bounds__(kBatchBlock) void batch_replay_kernel(BatchReplayArgs a) {
    batch_replay_lane<MG, false>(a);
}

template <int MG>
__global__ __launch_bounds__(kBatchBlock) void batch_carried_kernel(BatchReplayArgs a) {
    batch_replay_lane<MG, true>(a);
}

// rows [doff[p], doff[p] + cnt[p]) of the batch's MatchList = problem p's table, bucket-major
__global__ void batch_emit_kernel(const uint64_t* __restrict__ ord, const int64_t* __restrict__ pool,
                                  const uint32_t* __restrict__ mbase, const uint32_t* __restrict__ cnt,
                                  const uint64_t* __restrict__ doff, uint32_t G, uint64_t* __restrict__ out_len,
                                  int64_t* __restrict__ out_s) {
    const uint32_t p = blockIdx.x;
    const uint32_t n = cnt[p];
    const uint64_t* o = ord + (mbase[(uint64_t)p * G] >> 1);
    const uint64_t d = doff[p];
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
        const int64_t* row = pool + (uint64_t)(uint32_t)o[k] * (uint64_t)(G + 2);
        out_len[d + k] = (uint64_t)row[0];
        for (uint32_t g = 0; g < G; ++g) out_s[(d + k) * G + g] = row[2 + g];
    }
}

}  // namespace

hipError_t launch_batch_gap(const char* ascii, uint64_t lo, uint64_t hi, unsigned long long* d_first, hipStream_t st) {
    if (hi <= lo) return hipSuccess;
    const uint64_t threads = (hi - lo + 15) / 16;
    hipLaunchKernelGGL(batch_gap_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st, ascii, lo, hi,
                       d_first);
    return hipGetLastError();
}

hipError_t launch_batch_keys(const char* ascii, const uint64_t* aoff, const uint32_t* mbase, uint32_t nseg, uint32_t G,
                             uint32_t N, const SeedSpec& ss, int kbits, uint64_t* keys, hipStream_t st) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(batch_keys_kernel, dim3((uint32_t)(((uint64_t)N + 255) / 256)), dim3(256), 0, st, ascii, aoff, mbase, nseg, G, N,
                       ss, kbits, keys);
    return hipGetLastError();
}

// one round on the carried tables (b.ord_base set)
static hipError_t launch_batch_carried(const BatchReplayArgs& a, dim3 grid, dim3 block, hipStream_t st) {
    if (a.G <= 2) hipLaunchKernelGGL(batch_carried_kernel<2>, grid, block, 0, st, a);
    else if (a.G <= 4) hipLaunchKernelGGL(batch_carried_kernel<4>, grid, block, 0, st, a);
    else if (a.G <= 8) hipLaunchKernelGGL(batch_carried_kernel<8>, grid, block, 0, st, a);
    else if (a.G <= 16) hipLaunchKernelGGL(batch_carried_kernel<16>, grid, block, 0, st, a);
    else if (a.G <= 32) hipLaunchKernelGGL(batch_carried_kernel<32>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(batch_carried_kernel<64>, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_replay(const BatchReplay& b, hipStream_t st) {
    if (b.B == 0) return hipSuccess;
    BatchReplayArgs a{b.sk,  b.sv,     b.keys, b.mbase, b.nlen, b.order, b.ord, b.pool,       b.pool_cap, b.pool_n,
                      b.cnt, b.probes, b.coll, b.flag,  b.B,    b.G,     b.L,   b.kbits,      b.table_size,
                      b.masked, b.seq_mask, b.ord_base, b.ord_cap};
    const dim3 grid((b.B + kBatchBlock - 1) / kBatchBlock), block(kBatchBlock);
    if (b.ord_base) return launch_batch_carried(a, grid, block, st);
    if (b.G <= 2) hipLaunchKernelGGL(batch_replay_kernel<2>, grid, block, 0, st, a);
    else if (b.G <= 4) hipLaunchKernelGGL(batch_replay_kernel<4>, grid, block, 0, st, a);
    else if (b.G <= 8) hipLaunchKernelGGL(batch_replay_kernel<8>, grid, block, 0, st, a);
    else if (b.G <= 16) hipLaunchKernelGGL(batch_replay_kernel<16>, grid, block, 0, st, a);
    else if (b.G <= 32) hipLaunchKernelGGL(batch_replay_kernel<32>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(batch_replay_kernel<64>, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_emit(const uint64_t* ord, const int64_t* pool, const uint32_t* mbase, const uint32_t* cnt,
                             const uint64_t* doff, uint32_t B, uint32_t G, uint64_t* out_len, int64_t* out_s,
                             hipStream_t st) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(batch_emit_kernel, dim3(B), dim3(64), 0, st, ord, pool, mbase, cnt, doff, G, out_len, out_s);
    return hipGetLastError();
}

}  // namespace mums
