// dtof_shade_res0.hip -- instantiations of k_shade (dtof_shade.h): the resident first-bounce kernel (Domino: TLAS and small records in LDS, one persistent block per CU), diffuse scenes.
#include "dtof_shade.h"

namespace dtof {

// the resident kernel of one film at 16 waves (Domino, C4) compiled with the frame plan's constants (dtof_kernels.h: kFact*)
static void launch_resident_facts(const ShadeLaunch &L) {
    static std::atomic<uint32_t> attr_lds[64];
    const auto kernel = k_shade<false, 2, false, 1, true, 0, 16, false, kResidentFacts>;
    raise_dynamic_lds(attr_lds, { (const void *) kernel }, L.lds);
    hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(16 * 64), L.lds, L.stream, L.args);
}

uint32_t launch_shade_resident0(bool area, bool k4, const ShadeLaunch &L) {
    // taken when the launch satisfies every fact of the mask, the generic instantiations below otherwise
    if (kResidentFacts != 0 && !area && !k4 && L.waves == 16 && !L.args.rp.res_half && (L.facts & kResidentFacts) == kResidentFacts) { launch_resident_facts(L); return kResidentFacts; }
    if (area) { if (k4) launch_resident_variant<true, kMaxOffsets, 0>(L); else launch_resident_variant<true, 1, 0>(L); }
    else      { if (k4) launch_resident_variant<false, kMaxOffsets, 0>(L); else launch_resident_variant<false, 1, 0>(L); }
    return 0u;
}

}  // namespace dtof
