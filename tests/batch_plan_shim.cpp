// TEST INFRASTRUCTURE ONLY: libmems_amd/csrc/batch_plan.h compiled with g++, so the routing plan of
// mums_find_batch / mums_anchor_batch is held to tests/test_batch_plan_cpu.py without a device.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../libmems_amd/csrc/batch_plan.h"

// Outputs: recs (R * B), routed, order, obase, ocap (B each), mbase (R * (B * G + 1)), N, Nall (R each),
// scalars = {lanes, ord_words}.  Returns the plan's status; past kOk only scalars[0] is written.
extern "C" int batch_plan_run(uint32_t B, uint32_t G, const uint64_t* seq_off, uint32_t R, const int32_t* L,
                              const int32_t* kbits, uint64_t cap, int no_split, double lane_us, double alone_us,
                              uint64_t* recs, uint8_t* routed, uint32_t* order, uint32_t* mbase, uint64_t* N, uint64_t* Nall,
                              uint32_t* obase, uint32_t* ocap, uint64_t* scalars) {
    std::vector<mums::batch::Round> rounds(R);
    for (uint32_t r = 0; r < R; ++r) rounds[r] = {L[r], kbits[r]};
    const mums::batch::Plan pl = mums::batch::make_plan(B, G, seq_off, rounds, cap, no_split != 0, {lane_us, alone_us});
    scalars[0] = pl.lanes ? 1 : 0;
    if (pl.status != mums::batch::kOk) return (int)pl.status;
    scalars[1] = pl.ord_words;
    std::copy(pl.recs.begin(), pl.recs.end(), recs);
    std::copy(pl.routed.begin(), pl.routed.end(), routed);
    std::copy(pl.order.begin(), pl.order.end(), order);
    std::copy(pl.obase.begin(), pl.obase.end(), obase);
    std::copy(pl.ocap.begin(), pl.ocap.end(), ocap);
    for (uint32_t r = 0; r < R; ++r) {
        std::copy(pl.mbase[r].begin(), pl.mbase[r].end(), mbase + (uint64_t)r * ((uint64_t)B * G + 1));
        N[r] = pl.N[r];
        Nall[r] = pl.Nall[r];
    }
    return 0;
}
