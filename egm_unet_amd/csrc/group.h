// Launch groups: INDEPENDENT convolutions recorded between egm_group_begin() and egm_group_end() and launched together -- those that
// run the same kernel instantiation as ONE launch whose workgroups are split between the members by a block-index prefix.
//
// The parallel branches of EdgeEnhancedGRFB (src/EGM-UNet.py:1256-1278) put three convolutions of 16..128 channels side by side at
// every depth; at the 64^2 and 32^2 levels each of them has 32-256 workgroups for 256 CUs (two resident per CU), so three launches
// in a row leave most of the chip idle three times.  Independent branches on forked streams inside a captured graph are no answer on
// this ROCm (2x slower); one launch that carries all three is.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>

constexpr int EGM_GROUP_MAX = 4;        // members of one merged launch

struct EgmGroupRec {
    // launches recs[0..n) (n <= EGM_GROUP_MAX, all recorded by the same instantiation) on st
    int (*launch)(const EgmGroupRec* recs, int n, hipStream_t st);
    alignas(16) unsigned char params[384];   // the kernel's parameter struct, copied
    int G;                                    // pixel groups (kernels that take it beside the struct)
    int grid;                                 // workgroups of this member (multiple of 8: XCD alignment of the next member)
    size_t smem;                              // dynamic LDS bytes
};

bool egm_group_recording();
void egm_group_set_recording(bool on);      // pause / resume an open group (a launch whose result is consumed at once)
void egm_group_push(const EgmGroupRec& r);

// A merged launch passes ONE struct  M = { P p[EGM_GROUP_MAX]; <per-member extras>; int blk0[EGM_GROUP_MAX + 1]; int n; }  by value;
// member i owns the flat blocks [blk0[i], blk0[i+1]).
// Host: fill it from recs[0..n) -- parameters copied, blk0 = prefix sum of the members' grids (multiples of 8 where the kernel maps
// blocks to XCDs: every member starts on XCD 0), the unused members padded with a copy of member 0 that owns no block.  extras(i, rec)
// sets member i's extras (rec == nullptr for the padding).  Returns the largest dynamic LDS size of the members.
template <typename P, typename M, typename Extras>
size_t egm_group_fill(M& m, const EgmGroupRec* recs, int n, Extras extras) {
    size_t smem = 0;
    m.n = n; m.blk0[0] = 0;
    for (int i = 0; i < n; ++i) {
        memcpy(&m.p[i], recs[i].params, sizeof(P));
        m.blk0[i + 1] = m.blk0[i] + recs[i].grid;
        extras(i, &recs[i]);
        if (recs[i].smem > smem) smem = recs[i].smem;
    }
    for (int i = n; i < EGM_GROUP_MAX; ++i) { m.p[i] = m.p[0]; m.blk0[i + 1] = m.blk0[n]; extras(i, nullptr); }
    return smem;
}
// Device: declares `int i` = the member that owns this workgroup (flat block index blockIdx.x).  A statement macro, not a function: a
// helper function is optimised on its own before it is inlined (a 32-bit search loop that returns an int), the kernel then indexes
// m.p[i] differently, and every merged kernel's code changes; the macro is the loop as the kernels had it.
#define EGM_GROUP_MEMBER(m, i) \
    int i = 0;                 \
    while (i + 1 < (m).n && (int)blockIdx.x >= (m).blk0[i + 1]) ++i
