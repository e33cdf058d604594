// dtof_shade_spec2.hip -- instantiations of k_shade (dtof_shade.h): every BSDF + blendbsdf / two-BSDF twosided (SPEC = 2: the BSDF chain loops over two records).
#include "dtof_shade.h"

namespace dtof {

void launch_shade_spec2(bool k4, const ShadeLaunch &L) {
    if (k4) launch_shade_variant<true, kMaxOffsets, true, 2>(L); else launch_shade_variant<true, 1, true, 2>(L);
}

// dtof_bsdf_eval_ex, spec = 2 (k_bsdf_eval in dtof_shade.h)
void launch_bsdf_eval_2(const uint8_t *scene, uint32_t shape_index, const float *in, float *out, uint32_t n, hipStream_t s) {
    launch_bsdf_eval_spec<2>(scene, shape_index, in, out, n, s);
}

// dtof_emitter_eval, level 5 (k_emitter_eval in dtof_shade.h)
void launch_emitter_eval_spec2(const uint8_t *scene, int level, int mode, uint32_t index, float pmf, const float *in, float *out, uint32_t n, hipStream_t s) {
    launch_emitter_eval_level<true, true, 2>(scene, mode, index, pmf, in, out, n, s);
}

}  // namespace dtof
