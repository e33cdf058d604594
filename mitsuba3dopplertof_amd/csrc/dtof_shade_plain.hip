// dtof_shade_plain.hip -- instantiations of k_shade (dtof_shade.h): rectangle-only diffuse scenes (MESH = false, SPEC = 0): the headline kernels of the Cornell-wall benchmark.
#include "dtof_shade.h"

namespace dtof {

// The headline kernel (cornell_wall, C2 / C3: the staged first-bounce kernel of one film without area emitters) compiled with the frame plan's constants
// (dtof_kernels.h: kFact*): taken when the launch satisfies every fact of its mask and has the mask's shape fields, if it has any (facts_hold).  A kernel compiled
// with kFactFlat has no traversal stack: its launch carries no stack column (ShadeLaunch::lds_flat).
template <uint32_t FACTS> static uint32_t launch_headline(const ShadeLaunch &L) {
    if (FACTS == 0 || !facts_hold(L.facts, FACTS)) return 0u;
    hipLaunchKernelGGL((k_shade<true, 2, false, 1, false, 0, 0, false, FACTS>), dim3(L.grid), dim3(kShadeBlock), (FACTS & kFactFlat) ? L.lds_flat : L.lds, L.stream, L.args);
    return FACTS;
}
uint32_t launch_shade_plain(bool area, bool k4, const ShadeLaunch &L) {
    // The most specific kernel whose mask holds: C2's at three inline iterations, whose pairs share their BSDF samples (kHeadlinePairFacts), then C2's with its sampling
    // and modulation routes and the shape of its flat table compiled in (kHeadlineShapeFacts), then the
    // one with the routes for a table of any other shape (kHeadlineC2Facts), then the one that splats whatever the routes (kFactFusedSplat), then the one that leaves
    // the film to the splat kernels (C3, box filters); the generic instantiation below otherwise
    if (!area && !k4 && L.staged && L.mode == 2) {
        if (uint32_t ran = launch_headline<kHeadlinePairFacts>(L)) return ran;
        if (uint32_t ran = launch_headline<kHeadlineShapeFacts>(L)) return ran;
        if (uint32_t ran = launch_headline<kHeadlineC2Facts>(L)) return ran;
        if (uint32_t ran = launch_headline<kHeadlineFusedFacts>(L)) return ran;
        if (uint32_t ran = launch_headline<kHeadlineFacts>(L)) return ran;
    }
    if (area) { if (k4) launch_shade_variant<true, kMaxOffsets, false, 0>(L); else launch_shade_variant<true, 1, false, 0>(L); }
    else      { if (k4) launch_shade_variant<false, kMaxOffsets, false, 0>(L); else launch_shade_variant<false, 1, false, 0>(L); }
    return 0u;
}

// dtof_bsdf_eval_ex, spec = 0 (k_bsdf_eval in dtof_shade.h)
void launch_bsdf_eval_0(const uint8_t *scene, uint32_t shape_index, const float *in, float *out, uint32_t n, hipStream_t s) {
    launch_bsdf_eval_spec<0>(scene, shape_index, in, out, n, s);
}

// dtof_emitter_eval, levels 0 (no area emitters), 1 (area emitters) and 6 (level 0 under the kFactOneEmitter fact of the headline kernels) (k_emitter_eval in dtof_shade.h)
void launch_emitter_eval_plain(const uint8_t *scene, int level, int mode, uint32_t index, float pmf, const float *in, float *out, uint32_t n, hipStream_t s) {
    if (level == 1) launch_emitter_eval_level<true, false, 0>(scene, mode, index, pmf, in, out, n, s);
    else if (level == 6) launch_emitter_eval_level<false, false, 0, true>(scene, mode, index, pmf, in, out, n, s);
    else launch_emitter_eval_level<false, false, 0>(scene, mode, index, pmf, in, out, n, s);
}

}  // namespace dtof
