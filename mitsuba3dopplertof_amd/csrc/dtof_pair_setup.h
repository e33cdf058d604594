// dtof_pair_setup.h -- a correlated pair's share of lane generation, evaluated once per pair (DTOF_PAIR_SETUP, dtof_kernels.h).
// Under kFactsLaneSplit the path stream, its two jitter draws, the sample position and the camera ray are the same in lanes 2k and 2k + 1 (generate_pair_part,
// dtof_sampling.h).  One evaluation is one dependent chain, so the two lanes of a pair cannot share it inside a chunk; two CHUNKS can.  A block walks the 64-lane chunks
// of its segment in sequence: at every even chunk lane L evaluates the piece for pair L >> 1 of this chunk (L even) or of the chunk after it (L odd), the results stay in
// registers over both chunks (`carried`), and in each chunk every lane fetches its pair's values from the lane that holds them -- the even lane of the pair in the even
// chunk, the odd lane in the odd one (ds_bpermute_b32; DTOF_PAIR_SETUP_BPERMUTE=0: DPP moves behind one wave-uniform branch).  A tail chunk without a partner needs no guard: its odd lanes compute values nobody fetches.
// k_shade (dtof_shade.h) and the array entry (dtof_pair_setup.hip; dtof_pair_setup_lanes of include/dtof.h) run the same functions.
#pragma once
#include "dtof_kernels.h"
#include "dtof_sampling.h"

namespace dtof {

// the facts of kHeadlinePairFacts lane generation reads: what the array entry's kernels are compiled with, and what dtof_pair_setup_lanes checks a scene against
constexpr uint32_t kPairSetupLaneFacts = kFactsLaneSplit | kFactPow2Strata;
static_assert(kHeadlinePairFacts == 0 || (kHeadlinePairFacts & kPairSetupLaneFacts) == kPairSetupLaneFacts, "the headline kernel generates its lanes under these facts");
constexpr uint32_t kPairChunk = 64;        // lanes of a chunk: one wave (k_shade: kShadeBlock)
constexpr uint32_t kPairSetupWords = 16;   // per lane: pos[2], time, o[3], d[3], maxt, path state (lo, hi), path selector, 0, 0, 0
// Lanes [lane_base, lane_base + n_lanes) of rp in 512-lane segments of 64-lane chunks, one block per segment as the shade launch walks them; form 0: generate_lane per
// lane, form 1: the chunk-pair form.  out: kPairSetupWords words per lane.  The caller has checked the facts, the alignment of the range and its size.
void launch_pair_setup_lanes(const RenderParams &rp, int form, uint32_t *out, hipStream_t s);

constexpr uint32_t kPairPartWords = 12;   // the carried set: o, d, maxt, pos, the path state after the two draws, its selector
DTOF_D PairPart pair_part_zero() {
    PairPart p; p.o = mk(0.f, 0.f, 0.f); p.d = mk(0.f, 0.f, 1.f); p.maxt = 0.f; p.pos = make_float2(0.f, 0.f); p.path_state = 0ull; p.path_sel = 0u;
    return p;
}
// Every lane reads its pair's values from the even lane of the pair (ODD false: quad_perm [0, 0, 2, 2]) or from the odd one ([1, 1, 3, 3]) -- the DPP forms of (j)
// and (k), which take their control as an immediate: two texts behind one wave-uniform branch.  BPERMUTE: the same lanes through ds_bpermute_b32, which takes no
// VALU slot and no LDS allocation and reads its source lane from a register -- one text for both chunks, no branch.
DTOF_D void pair_part_words(const PairPart &c, uint32_t (&w)[kPairPartWords]) {
    w[0] = f2u(c.o.x); w[1] = f2u(c.o.y); w[2] = f2u(c.o.z); w[3] = f2u(c.d.x); w[4] = f2u(c.d.y); w[5] = f2u(c.d.z); w[6] = f2u(c.maxt); w[7] = f2u(c.pos.x); w[8] = f2u(c.pos.y);
    w[9] = (uint32_t) c.path_state; w[10] = (uint32_t) (c.path_state >> 32); w[11] = c.path_sel;
}
DTOF_D PairPart pair_part_of_words(const uint32_t (&r)[kPairPartWords]) {
    PairPart p;
    p.o = mk(u2f(r[0]), u2f(r[1]), u2f(r[2])); p.d = mk(u2f(r[3]), u2f(r[4]), u2f(r[5])); p.maxt = u2f(r[6]); p.pos = make_float2(u2f(r[7]), u2f(r[8]));
    p.path_state = (uint64_t) r[9] | ((uint64_t) r[10] << 32); p.path_sel = r[11];
    return p;
}
template <bool ODD>
DTOF_D PairPart pair_fetch_dpp(const PairPart &c) {
    uint32_t w[kPairPartWords], r[kPairPartWords];
    pair_part_words(c, w);
#pragma unroll
    for (uint32_t i = 0; i < kPairPartWords; ++i) r[i] = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) w[i], ODD ? 0xf5 : 0xa0, 0xf, 0xf, false);
    return pair_part_of_words(r);
}
DTOF_D PairPart pair_fetch_bpermute(const PairPart &c, uint32_t lane_id, bool odd) {
    uint32_t w[kPairPartWords], r[kPairPartWords];
    pair_part_words(c, w);
    const int addr = (int) (((lane_id & ~1u) | (odd ? 1u : 0u)) << 2);   // the byte address of the source lane
#pragma unroll
    for (uint32_t i = 0; i < kPairPartWords; ++i) r[i] = (uint32_t) __builtin_amdgcn_ds_bpermute(addr, (int) w[i]);
    return pair_part_of_words(r);
}
// One chunk of a segment's walk.  first: the global lane index of the chunk's lane 0 (uniform, a multiple of 64); second (uniform): the chunk's index in its segment is
// odd; carried: the block's loop-carried pair values, written in the even chunks.  The whole wave is active (kFactWavePixel).  Returns what generate_lane returns for
// lane first + lane_id, bit for bit: the same functions on the same inputs, evaluated in another lane.
template <uint32_t FACTS, bool BPERMUTE = DTOF_PAIR_SETUP_BPERMUTE != 0>
DTOF_D PrimaryLane pair_setup_chunk(const RenderParams &rp, uint32_t first, uint32_t lane_id, bool second, PairPart &carried) {
    const PixelInfo here = pixel_info<true>(rp, first >> rp.spp_log2);
    if (!second) {   // the setup pass: the even lane does this chunk's pair, the odd lane the next chunk's -- whose pixel need not be in the same row
        const PixelInfo next = pixel_info<true>(rp, (first + kPairChunk) >> rp.spp_log2);
        const bool odd = lane_id & 1u;
        carried = generate_pair_part<FACTS>(rp, first + (odd ? kPairChunk : 0u) + lane_id, odd ? next.posx : here.posx, odd ? next.posy : here.posy);
    }
    PairPart pp;
    if (BPERMUTE) pp = pair_fetch_bpermute(carried, lane_id, second);
    else if (second) pp = pair_fetch_dpp<true>(carried); else pp = pair_fetch_dpp<false>(carried);
    const LanePart lp = generate_lane_part<FACTS>(rp, first + lane_id, here.perm_seed);
    PrimaryLane pl;
    pl.ray_a = make_float4(pp.o.x, pp.o.y, pp.o.z, lp.time);
    pl.ray_b = make_float4(pp.d.x, pp.d.y, pp.d.z, pp.maxt);
    pl.main = lp.main; pl.path.state = pp.path_state; pl.path.inc = ((uint64_t) pp.path_sel << 1) | 1u; pl.pos = pp.pos;
    return pl;
}

}  // namespace dtof
