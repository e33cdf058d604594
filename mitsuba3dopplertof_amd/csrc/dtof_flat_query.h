// dtof_flat_query.h -- launcher of the flat-table ray query over arrays (dtof_flat_query.hip; dtof_flat_query of include/dtof.h).  Kept out of dtof_kernels.h like
// dtof_reconstruct.h and dtof_film64.h: only the host orchestration reads it, and the translation units of the render kernels do not change with it.
#pragma once
#include "dtof_kernels.h"
#include "dtof_zrow_mfma.h"

namespace dtof {

// The table's facts each form of the query compiles trace_flat with -- what k_shade hands it, FACTS & kFactsFlatTable of the generic kernels (0), of the one-wall
// kernels (kHeadlineC2Facts) and of the headline's shaped kernel (kHeadlineShapeFacts)
constexpr uint32_t kFlatQueryForms = 3;
constexpr uint32_t flat_query_facts(int form) { return form == 2 ? kHeadlineShapeFacts & kFactsFlatTable : form == 1 ? (uint32_t) kFactOneWall : 0u; }
// ... and, for the launcher only (dtof_flat_query_pairs; dtof_flat_query refuses it), the shaped walk's pair form: rays 2k and 2k + 1 equal but for their times
constexpr int kFlatQueryPairs = 3;
constexpr bool kFlatQueryPairsBuilt = pair_walk_shape(flat_query_facts(2));   // the form is written for one shape (trace_flat: PAIR_RAYS)
// ... and its form with the plain rectangles' z rows from the matrix cores (dtof_flat_query_zrow; trace_flat: ZROW), which also writes those rows to zrow8 if given
constexpr int kFlatQueryZrow = 4;
constexpr bool kFlatQueryZrowBuilt = zrow_mfma_shape(flat_query_facts(2));
// One ray per lane, blocks of one wave: rays = o[3], d[3], time, maxt; closest hit: out3 = t, u, v (inf, 0, 0 on a miss), ids = the object or -1; occlusion: ids = 1 / 0.
// flat_off, flat_objects, memo_obj: RenderParams::flat_off / flat_objects / memo_obj as a frame plan sets them.  Throws when the blob does not fit the LDS stage.
void launch_flat_query(const uint8_t *scene, uint32_t scene_bytes, uint32_t flat_off, uint32_t flat_objects, uint32_t memo_obj, int form, bool any,
                       const float *rays, float *out3, int32_t *ids, uint32_t n, hipStream_t s, float *zrow8 = nullptr);

}  // namespace dtof
