// dtof_pair_setup.hip -- lane generation over arrays, in the two forms C2's kernel can run it (dtof_pair_setup.h): generate_lane per lane, and the chunk-pair form in
// which a pair's piece is evaluated once for the pairs of two chunks.  The walk is the shade launch's -- one block of one wave per 512-lane segment, its 64-lane chunks in
// sequence -- and the device functions are the ones k_shade calls.  A translation unit of its own: the render kernels' units do not see it.
#include "dtof_device.h"
#include "dtof_pair_setup.h"

namespace dtof {

template <int FORM>
__global__ __launch_bounds__(kShadeBlock) void k_pair_setup_lanes(RenderParams rp, uint32_t *out) {
    constexpr uint32_t FACTS = kPairSetupLaneFacts;
    const uint32_t seg = blockIdx.x, lane_id = threadIdx.x;
    const uint32_t count = seg_count(nullptr, seg, rp.n_lanes);
    PairPart carried = pair_part_zero();
    for (uint32_t cbase = 0; cbase < count; cbase += kShadeBlock) {   // (count - cbase >= 64 in every chunk: the host refuses ranges that are not whole chunks)
        const uint32_t l = seg * kSeg + cbase + lane_id;
        PrimaryLane pl;
        if (FORM == 1) pl = pair_setup_chunk<FACTS>(rp, rp.lane_base + seg * kSeg + cbase, lane_id, ((cbase >> 6) & 1u) != 0, carried);
        else pl = generate_lane<true, FACTS>(rp, global_lane<FACTS>(rp, rp.lane_base + l), true, rp.lane_base + l);
        uint4 *const w = (uint4 *) (out + (size_t) l * kPairSetupWords);
        w[0] = make_uint4(f2u(pl.pos.x), f2u(pl.pos.y), f2u(pl.ray_a.w), f2u(pl.ray_a.x));
        w[1] = make_uint4(f2u(pl.ray_a.y), f2u(pl.ray_a.z), f2u(pl.ray_b.x), f2u(pl.ray_b.y));
        w[2] = make_uint4(f2u(pl.ray_b.z), f2u(pl.ray_b.w), (uint32_t) pl.path.state, (uint32_t) (pl.path.state >> 32));
        w[3] = make_uint4((uint32_t) (pl.path.inc >> 1), 0u, 0u, 0u);
    }
}

void launch_pair_setup_lanes(const RenderParams &rp, int form, uint32_t *out, hipStream_t s) {
    if (!rp.n_lanes) return;
    const uint32_t grid = nseg(rp.n_lanes);
    if (form == 1) hipLaunchKernelGGL((k_pair_setup_lanes<1>), dim3(grid), dim3(kShadeBlock), 0, s, rp, out);
    else hipLaunchKernelGGL((k_pair_setup_lanes<0>), dim3(grid), dim3(kShadeBlock), 0, s, rp, out);
}

}  // namespace dtof
