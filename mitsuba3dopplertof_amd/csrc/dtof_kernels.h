// dtof_kernels.h -- kernel parameter blocks and queue layout shared by the host
// orchestration (dtof_render.hip, dtof_abi_*.hip through dtof_host.h) and the kernels (dtof_kernels.hip).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "dtof_math.h"

namespace dtof {

constexpr uint32_t kChunkBlocks = 8; // 64-lane chunks of a 512-lane queue segment (RenderParams::chunk_blocks)
constexpr uint32_t kMaxInline = 4;  // iterations of the bounce loop the fused first-bounce kernel may run itself (RenderParams::inline_iters)
constexpr int kMaxOffsets = 4;      // modulation variants (hetero_frequency, hetero_offset, w_g) evaluated per traversal (K), one film each

// Everything a kernel needs besides the scene blob and the queues; passed by value.
struct RenderParams {
    // ---- camera (PerspectiveCamera, src/sensors/perspective.cpp:172-279)
    float s2c[16];                  // sample_to_camera
    float cam_to_world[12];
    float near_clip, far_clip, shutter_open, shutter_open_time;
    int32_t orthographic;                    // OrthographicCamera (src/sensors/orthographic.cpp:169-196)
    float aperture_radius, focus_distance;   // ThinLensCamera (src/sensors/thinlens.cpp:257-305); aperture_radius == 0: perspective
    // ---- film (lane -> pixel mapping src/render/integrator.cpp:273-290; splat imageblock.cpp:414-531)
    int32_t crop_x, crop_y, crop_w, crop_h;
    float scale_x, scale_y, offset_x, offset_y;   // render_sample: scale = 1/crop_size, offset = -crop_offset*scale
    int32_t filter; float filter_radius, inv_radius;
    float gauss_coeff[10];                        // GaussianFilter's Remez fit, scaled and shifted like gaussian.cpp:60-89
    float filter_b, filter_c;       // mitchell: B, C (src/rfilters/mitchell.cpp)
    // ---- sampler (src/samplers/correlated.cpp, src/render/sampler.cpp)
    uint32_t base_seed, seed, seed_value;         // seed_value = base_seed + seed
    uint32_t spp, spp_log2;                       // spp_log2 = 0xffffffff when spp is not a power of two
    uint32_t tcn, pcn;
    int32_t time_sampling; float antithetic_shift; int32_t stratify;
    uint32_t n_stratum; float inv_n_stratum, inv_tcn;
    // ---- integrator (src/integrators/dopplertofpath.cpp:19-77)
    float T, amp, g_1, g_0;
    // per film: the illumination frequency with the path-length prefactor that follows from it, the heterodyne frequency and the phase offset (only
    // eval_modulation_weight reads the four); n_offsets = K.  A one-film kernel reads element 0.
    float w_g[kMaxOffsets], phi_coef[kMaxOffsets], w_d[kMaxOffsets], phase[kMaxOffsets]; int32_t n_offsets;
    int32_t wave_type, low_pass;
    uint32_t path_correlation_depth, max_depth, rr_depth;
    int32_t has_area;                             // scene has area emitters: emitter-hit term + prev_si / prev_bsdf_pdf state
    int32_t sampler_kind, jitter; float inv_spp;  // SamplerKind; timestratified: jitter, 1 / sample_count (timestratified.cpp:78-82)
    int32_t has_spec;                             // scene has delta BSDFs (conductor / dielectric): eta and prev_bsdf_delta become per-lane state; 2: ... and blendbsdf
    int32_t has_tris;                             // scene has triangle meshes (selects the kernel instantiations that carry mesh code)
    int32_t has_analytic;                         // the scene has spheres / disks / cylinders (the eight-wave ray kernels carry triangle and rectangle code only)
    uint32_t n_tlas_nodes;                        // nodes of the top-level BVH (the eight-wave ray kernels keep up to kTlasLds8 of them in LDS)
    uint32_t res_half;                            // resident stage: the LDS planes hold half-float node records (a TLAS of kResidentNodes + 1 .. 2 * kResidentNodes nodes)
    int32_t has_nodes16;                          // the blob carries the half-float copy of the node array (BlobHeader::off_nodes16)
    int32_t has_blas;                             // some mesh is traversed through its own BLAS: the unstaged k_trace / k_shadow run one wave per block
    int32_t integrator;                           // 0 dopplertofpath, 1 path (src/integrators/path.cpp), 2 velocity (velocity.cpp)
    // ---- batch
    uint32_t lane_base, n_lanes;                  // this batch covers (virtual) lanes [lane_base, lane_base + n_lanes)
    // striped shards (dtof_render_stripes): virtual row v of this shard is film row stripe_first + (v / stripe_rows) * stripe_period
    // + v % stripe_rows, and the GLOBAL lane index (what every RNG stream is a function of) follows from it.  stripe_rows == 0:
    // virtual = global (contiguous rows).
    uint32_t stripe_rows, stripe_period, stripe_first, lanes_per_row;
    // exact division by the launch-invariant divisors of the lane mappings (dtof_math.h: FastDiv)
    FastDiv d_spp, d_w, d_tcn, d_pcn, d_stratum, d_lanes_per_row, d_stripe_rows;
    // wavefronts of more than 2^32 - 1 lanes / samples_per_pass (integrator.cpp:121-124,227-245): pass `pass` of `n_passes`, each of
    // `spp` samples per pixel (= samples per wavefront); the sampler's streams are seeded in pass 0 and carried across the passes
    uint32_t pass, n_passes;
    uint32_t sample_count; FastDiv d_sample_count;   // Sampler::sample_count() of the whole render (spp = samples per wavefront = per pass)
    uint2 *pass_rng;                              // n_passes > 1: [lane - pass_first][3] = states of the main / time / path streams between passes
    uint32_t pass_first;                          // virtual lane the pass_rng array starts at
    int32_t has_env, hide_emitters; uint32_t env_index;   // `constant` environment emitter (scene.cpp:53-57), SamplingIntegrator::m_hide_emitters
    uint32_t chunk_blocks;                        // first-bounce kernel: blocks per 512-lane segment, 1 or 8 (small frames whose whole path runs inline)
    uint32_t res_units;                           // resident first-bounce kernel whose launch covers the whole path: work units a wave takes from the counter per 512-lane segment (1, 2, 4, 8)
    uint32_t inline_iters;                        // fused first-bounce kernel: iterations of the bounce loop it runs back to back with the path state in registers (1 .. kMaxInline)
    uint32_t flat_objects, flat_off;                        // fused pipeline, rectangle-only scenes of at most kFlatObjects objects: their number (trace_flat), else 0
    uint32_t memo_obj;                            // fused pipeline: the scene's only instance object (instance memo, dtof_traverse.h) or 0xffffffff
    int32_t want_valid;                           // the kernel that ends a path also writes its valid_ray flag to Queues::valid_out (alpha channel of an rgba film, lane dumps)
    float emitter_pmf;                            // m_emitter_pmf (scene.cpp:96) = 1 / emitter count, 0 without emitters: launch-invariant, divided once on the host (plan_frame)
    // The last iteration of this launch is TERMINAL: nothing continues any path after it (no further iteration runs, single pass, no null lobe that could still
    // change valid_ray), so k_shade drops the half of the bounce nobody reads -- BSDF sampling, the draws behind the emitter sample, continuation ray, throughput /
    // russian roulette, the advance of both streams -- and, where the iteration has no emitter sampling either (active_next false), everything behind the emitter-hit term
    int32_t terminal;
    // A pixel list (RenderRequest::pixels; adaptive passes, regions of interest): n strictly ascending flat indices y * crop_w + x of the crop window, device memory.  The
    // launch's virtual lanes are [0, n * spp); virtual lane v is GLOBAL lane pixels[v / spp] * spp + v % spp (global_lane, dtof_sampling.h), so a listed pixel's lanes
    // are, stream for stream, those of the dense render with the same seed.  nullptr: no list.  Batches are whole pixels (lane_base is a multiple of spp).
    const uint32_t *pixels;
};

// SoA wavefront state for one batch (device pointers; all arrays have `capacity` entries and are
// indexed by the lane's position inside the batch).
struct Queues {
    float4 *ray_a;       // o.xyz, time
    float4 *ray_b;       // d.xyz, maxt
    uint4  *hit;         // t, u, v (float bits), prim
    float  *hit_t;       // rectangle-only scenes: t alone replaces `hit`
    uint32_t *hit_id;    // object (low id_shift bits) | shape-in-group (the bits above); 0xffffffff = miss
    float4 *st_a;        // throughput.xyz, path_length
    float4 *st_b;        // prev_si.p, prev_bsdf_pdf (only touched when the scene has area emitters)
    uint4  *rng_a;       // rng.state (lo,hi), rng_path.state (lo,hi)
    float2 *st_c;        // SPEC: (eta along the path, prev_bsdf_delta | valid_ray << 1 as a float 0 .. 3)
    float4 *valid_out;   // RenderParams::want_valid: (valid_ray ? 1 : 0, 0, 0, 0) of every finished path -- laid out like `res`, so the splat kernels accumulate the alpha film from it
    uint2  *rng_b;       // (main, path) stream selectors v1 of the TEA seeding: inc = (v1 << 1) | 1, constant per lane
    float4 *res;         // [K][capacity] accumulated result rgb (w unused)
    float2 *pos;         // sample position on the film
    float4 *sh_a;        // shadow ray o.xyz, maxt
    float4 *sh_b;        // shadow ray d.xyz, time
    float4 *sh_c;        // [K][capacity] candidate result rgb, w = as_float(lane position)
    uint32_t *q[2];      // active-lane index queues (ping-pong), segmented: entry j of segment S at S*kSeg + j
    uint32_t *counts;    // [iteration][2][n_segments]: survivors / shadow rays per segment
    uint4 *cand;         // DEFER (ray kernels of large meshes): up to four objects a ray's TLAS walk put aside, by lane (k_trace) / by shadow slot (k_shadow); nullptr = no second launch
    uint32_t *defer_idx; // ... the lanes / shadow slots of a segment that have some, entry j of segment S at S*kSeg + j, and
    uint32_t *defer_cnt; // ... how many (zeroed before each first launch)
    uint32_t *seg_counter;   // resident first-bounce kernel: next segment to hand out (zeroed before the launch)
    uint32_t capacity;
    uint32_t xcd_remap;  // unstaged ray kernels: XCD-aware block order (dtof_kernels.hip: xcd_remap); 0 = block b traces segment b
    uint32_t id_shift;   // bits of hit_id that hold the object index: 24 unless the scene needs more shapes per group than 8 bits hold (render_rows)
};

struct LaneDebug {       // mirrors orc_lane's comparable fields
    float sample_pos[2]; float time; float ray_o[3]; float ray_d[3]; float rgb[3]; float valid;
};

// The arguments of k_shade (dtof_shade.h) travel as ONE by-value block, read through the kernarg segment pointer.
struct ShadeArgs {
    const uint8_t *scene; uint32_t scene_bytes, stage_words; RenderParams rp; Queues q;
    const uint32_t *qin, *count_in; uint32_t *qout, *alive_out, *shadow_out; uint32_t depth, trace_next; LaneDebug *dbg;
    float *film; uint64_t film_stride;   // first-bounce kernel whose launch covers the whole path: it splats its lanes itself (k_shade, "fused splat"); nullptr: the splat kernels do
    uint32_t n_seg, res_small_off, res_small_words, res_memo;   // resident stage (RESW != 0): segments of the batch; byte offset / uint4 count of the record block copied to LDS; 1 = the instance memo has LDS
    uint32_t res_park_off;   // resident stage with several films: word offset (behind the memo) of the film-state columns, kParkWords words per thread behind the stack columns
};
static_assert(sizeof(ShadeArgs) == 920, "ShadeArgs is k_shade's kernarg block: its layout, order and types do not change (896 + the six floats that made RenderParams::w_g and ::phi_coef per film)");
// Resident kernels of several films keep the films' running results in LDS instead of registers (k_shade: RES_LDS): kParkWords of the 3 * kMaxOffsets floats per
// thread -- what Domino's stage leaves free of the CU's 160 KiB at 16 waves (64 KiB node planes + 3 KiB records + 48 KiB stack columns) -- the last one stays a register
constexpr uint32_t kParkWords = 11;
// DTOF_PARK (default 1): the resident ONE-film kernels at 16 waves (128 VGPRs, ~150 spilled) park the path state no traversal reads -- both PCG states with their
// stream selectors and throughput / path length, kParkState words -- in the same columns across the two traversals of an iteration instead of leaving them to the register
// allocator's spill code: scratch 200 -> 168 B per lane, C4 33.69 -> 33.26 ms (profiles/r05_k4_film_state.txt).  A scene whose stage no longer fits the CU's LDS with
// the columns at 16 waves takes 12 (ShadeLds::resident / plan_frame's step-down), where the kernels have 168 VGPRs and park nothing.
#ifndef DTOF_PARK
#define DTOF_PARK 1
#endif
constexpr uint32_t kParkState = 10, kParkRng = 6;   // one film: both streams + throughput / path length; several films (behind the kParkWords film words): the streams only
constexpr uint32_t kResidentNodes = 1024;   // TLAS nodes the resident stage holds (= kResNodes of dtof_traverse.h)
// instance memo (SceneView::memo, dtof_traverse.h): 12 words per thread, word k of thread t at memo[k * kMemoStride + t]
constexpr uint32_t kMemoStride = 64, kMemoWords = 12;

// The dynamic LDS of ONE k_shade launch, part by part in the kernel's order (bytes).  Whatever sizes that LDS on the host -- the plan's choice of a wave count, the
// launch, ShadeArgs::res_park_off -- reads it here; k_shade derives the same offsets from its template parameters and ShadeArgs (stage_words, memo_words, stack, park).
struct ShadeLds {
    uint32_t stage, memo;   // the staged scene blob, or the resident stage: four node planes + the record block; instance-memo columns of kMemoWords words per thread
    uint32_t stack, park;   // traversal-stack columns, one entry per thread and level; resident kernels: film-state / path-state columns (kParkWords, kParkState, kParkRng)
    constexpr uint32_t bytes() const { return stage + memo + stack + park; }
    constexpr uint32_t without_stack() const { return stage + memo + park; }   // a kernel compiled with kFactFlat has no traversal stack and is launched without the columns
    constexpr uint32_t park_off() const { return stack / 4u; }                 // ShadeArgs::res_park_off: the park columns lie this many words behind the memo
    static constexpr ShadeLds columns(uint32_t stage_words, uint32_t waves, uint32_t memo_columns, uint32_t stack_depth, bool entries16, uint32_t park_words) {   // waves of 64 threads; at least two stack levels
        return { stage_words * 16u, memo_columns * waves * kMemoWords * kMemoStride * 4u, (stack_depth < 2 ? 2u : stack_depth) * waves * 64u * (entries16 ? 2u : 4u), park_words * waves * 64u * 4u };
    }
    // The classic launch, one wave per block.  Split pipeline: the staged scene alone.  Fused: one memo column and the stack; a flat scene with ONE instance (one_instance:
    // fused, rectangle-only diffuse, rp.flat_objects != 0, rp.memo_obj set = k_shade's memo_m_lds) keeps the instance matrix in a second column and needs one stack level.
    static constexpr ShadeLds classic(uint32_t stage_words, bool fused, bool one_instance, uint32_t stack_depth) {
        return fused ? columns(stage_words, 1u, one_instance ? 2u : 1u, one_instance ? 1u : stack_depth, false, 0u) : ShadeLds { stage_words * 16u, 0u, 0u, 0u };
    }
    // The resident launch, `waves` waves per block: a memo column per wave if the scene has a memo object; with several films 16-bit stack entries (dtof_traverse.h:
    // encode_child16) and the film-state columns (k_shade: RES_LDS); at 16 waves the parked path state (PARK: one film kParkState words, several films the two streams)
    static constexpr ShadeLds resident(uint32_t small_words, uint32_t waves, bool memo, bool several_films, uint32_t stack_depth) {
        return columns(4u * kResidentNodes + small_words, waves, memo ? 1u : 0u, stack_depth, several_films, (several_films ? kParkWords : 0u) + (DTOF_PARK && waves == 16 ? (several_films ? kParkRng : kParkState) : 0u));
    }
};
// known totals: Domino's stage (171 record words, 12 stack levels), one film at 16 waves without / with a memo column, four films at 8 waves; cornell_wall's classic one-wall launch (a 214-word blob) with and without its stack column
static_assert(ShadeLds::resident(171, 16, false, false, 12).bytes() == 158384 && ShadeLds::resident(171, 16, true, false, 12).bytes() == 207536, "resident stage, one film");
static_assert(ShadeLds::resident(171, 8, false, true, 12).bytes() == 103088 && ShadeLds::resident(171, 8, false, true, 12).park_off() == 3072, "resident stage, four films");
static_assert(ShadeLds::classic(214, true, true, 5).bytes() == 10080 && ShadeLds::classic(214, true, true, 5).without_stack() == 9568, "classic one-wall launch");

// Plan facts (k_shade's FACTS template parameter): things the host fixed in the frame plan before a first-bounce launch, the same for every lane of it, that the kernel
// otherwise re-decides inside its chunk and bounce loops -- each a scalar load from the kernarg segment at its point of use, a wait that also drains the LDS reads, a
// branch, and registers kept alive for the side that is never taken.  A kernel instantiated with a mask reads the constant instead; render_rows (FramePlan::launch_facts)
// works out which facts a launch satisfies, and a launcher picks a specialised instantiation only when every fact of its mask holds.
enum : uint32_t {
    kFactSinglePass     = 1u << 0,   // rp.n_passes == 1 (and with it rp.pass == 0): no stream state is carried between passes
    kFactDopplerCorr    = 1u << 1,   // rp.integrator == 0 (dopplertofpath) and rp.sampler_kind == SAMPLER_CORRELATED
    kFactNoLaneOutput   = 1u << 2,   // dbg == nullptr and rp.want_valid == 0: neither the lane dump's camera rays nor valid_out are written
    kFactIdentityQueue  = 1u << 3,   // qin == nullptr and count_in == nullptr: lane j of segment S is lane S * kSeg + j, a segment's count follows from n_lanes
    kFactNoRoulette     = 1u << 4,   // rp.rr_depth > depth + rp.inline_iters: russian roulette is not reached by any iteration (its draw still advances the stream)
    kFactCorrelated     = 1u << 5,   // depth + rp.inline_iters < rp.path_correlation_depth: every iteration draws from the path-correlated stream
    kFactWholePath      = 1u << 6,   // trace_next == 0 and rp.terminal != 0: nothing is queued behind the launch, its last iteration is the terminal one
    kFactOneBlock       = 1u << 7,   // rp.chunk_blocks == 1: one block per 512-lane segment
    kFactOneEmitter     = 1u << 8,   // the scene has exactly one emitter
    kFactWavePixel      = 1u << 9,   // every chunk of every segment is a whole, 64-aligned wave of one pixel (k_shade: wave_pixel), proven from spp, lane_base and n_lanes
    // ... and facts of the scene the launch traces:
    kFactFlat           = 1u << 10,  // rp.flat_objects != 0: every ray query is trace_flat; the kernel has no traversal stack and its launch no stack column in LDS
    kFactOneWall        = 1u << 11,  // (with kFactFlat) the scene has exactly one instance object, it is rp.memo_obj and holds ONE rectangle (DFlatObject::instance == 2,
                                     // DFlatKinds::general == 0, ::memo == 1u << memo_obj), and its matrix sits in the lane's LDS column (k_shade: memo_m_lds)
    kFactFusedSplat     = 1u << 12,  // A.film != nullptr: the launch splats its lanes itself (plan_frame: fuse_splat_ok -- tent filter of radius in (0.5, 1], 64 spp, one film)
    // ... and the sampler's and the integrator's choices of a route: which VALUES the route reads (n_stratum, inv_tcn, amp, w_d, ...) stays run-time
    kFactStratifiedPairs = 1u << 13, // rp.time_sampling == TIME_STRATIFIED, rp.stratify != 0, rp.tcn == 2 and rp.pcn == 2, rp.shutter_open_time > 0, rp.spp > 1: no time stream,
                                     // next_time is its stratified route, pair and member of a sample are a shift and a mask
    kFactPow2Strata     = 1u << 14,  // rp.n_stratum is a power of two >= 2: permute_kensler_pow2 (dtof_math.h), no cycle-walking loop and no division
    kFactSineLowPass    = 1u << 15,  // rp.low_pass != 0 and rp.wave_type == WAVE_SIN: modulation_weight is amp * cos_(fmod_pos(w_d * t + phase + phi))
    kFactEmitterSampled = 1u << 16,  // depth + rp.inline_iters < rp.max_depth: every iteration of the launch samples an emitter (k_shade: active_next)
    kFactIdShift24      = 1u << 17,  // q.id_shift == 24
    // ... and the SHAPE of the one-wall flat table: a presence bit and two fields that are VALUES, not facts of one bit each -- see flat_shape_fact
    kFactFlatShape      = 1u << 18,  // (with kFactOneWall) bits 19 .. 22 hold rp.flat_objects (1 .. 8), bits 23 .. 25 rp.memo_obj (< rp.flat_objects)
    // ... and, above the shape fields, work the two lanes of a correlated pair can share:
    kFactPairSamples    = 1u << 26,  // rp.inline_iters == 3 under kFactWholePath, kFactWavePixel, kFactStratifiedPairs, kFactCorrelated, kFactDopplerCorr, kFactNoRoulette and
                                     // kFactOneEmitter: lanes 2k and 2k + 1 hold the same path stream, every draw of the loop comes from it, and iterations 0 and 1 sample
                                     // a BSDF while iteration 2 is the terminal one -- a diffuse-only point-light kernel reads two draws per sampling iteration and nothing else
};
// The shape fields: a launch's mask carries them whenever kFactOneWall holds and the table has at most 8 objects (FramePlan::launch_facts, read off the plan's blob);
// a kernel compiled with a shape is taken only by a launch whose fields EQUAL its own (facts_hold), every other shape falls back to the kernels without one.
constexpr uint32_t kFlatShapeCountShift = 19, kFlatShapeWallShift = 23, kFlatShapeMax = 8;
constexpr uint32_t kFlatShapeFields = kFactFlatShape | 0xfu << kFlatShapeCountShift | 0x7u << kFlatShapeWallShift;
constexpr uint32_t flat_shape_fact(uint32_t n_objects, uint32_t wall) {
    return n_objects >= 1 && n_objects <= kFlatShapeMax && wall < n_objects ? kFactFlatShape | n_objects << kFlatShapeCountShift | wall << kFlatShapeWallShift : 0u;
}
constexpr uint32_t flat_shape_count(uint32_t facts) { return (facts & kFactFlatShape) ? (facts >> kFlatShapeCountShift) & 0xfu : 0u; }
constexpr uint32_t flat_shape_wall(uint32_t facts) { return (facts >> kFlatShapeWallShift) & 0x7u; }
// does a launch that satisfies `launch` meet every fact of the mask `kernel` was compiled with?  The one-bit facts as a subset, the shape fields by equality.
constexpr bool facts_hold(uint32_t launch, uint32_t kernel) {
    return (launch & kernel & ~kFlatShapeFields) == (kernel & ~kFlatShapeFields) && (!(kernel & kFactFlatShape) || (launch & kFlatShapeFields) == (kernel & kFlatShapeFields));
}
constexpr uint32_t kFactsFlatTable = kFactOneWall | kFlatShapeFields;   // what of a kernel's mask trace_flat is instantiated with
static_assert(flat_shape_fact(5, 2) == 0x12c0000u && flat_shape_count(flat_shape_fact(5, 2)) == 5 && flat_shape_wall(flat_shape_fact(5, 2)) == 2 && flat_shape_fact(9, 2) == 0 && flat_shape_fact(5, 5) == 0, "shape fields");
// The facts of (h).  A kernel that carries any of them AND kFactWavePixel also takes the lane mappings kFactWavePixel proves -- global lane = virtual lane (no stripes), the
// pixel a shift of the wave's first lane by rp.spp_log2, the sample index a mask -- which the kernels compiled before (h) keep reading: their machine code does not move.
constexpr uint32_t kFactsSampling = kFactStratifiedPairs | kFactPow2Strata | kFactSineLowPass | kFactEmitterSampled | kFactIdShift24;
constexpr bool facts_lane_shifts(uint32_t facts) { return (facts & kFactWavePixel) != 0 && (facts & kFactsSampling) != 0; }
// the mask the headline kernel (dtof_shade_plain.hip) is compiled with; A/B of a subset: make variant NAME=x DEFS=-DDTOF_HEADLINE_FACTS=0x17
#ifndef DTOF_HEADLINE_FACTS
#define DTOF_HEADLINE_FACTS 0xfff
#endif
constexpr uint32_t kHeadlineFacts = DTOF_HEADLINE_FACTS;
// ... and a second instantiation with kFactFusedSplat on top: C2's kernel (the mask above also serves C3 and every frame that leaves the splat to the splat kernels);
// A/B without it: DEFS=-DDTOF_HEADLINE_FUSED=0
#ifndef DTOF_HEADLINE_FUSED
#define DTOF_HEADLINE_FUSED 1
#endif
constexpr uint32_t kHeadlineFusedFacts = DTOF_HEADLINE_FUSED ? (kHeadlineFacts | kFactFusedSplat) : 0u;
// ... and a third with the route facts of (h) on top of that: C2 again (stratified pairs, 32 strata, the sinusoidal low-pass weight), tried before them; C3 (antithetic_mirror)
// and whatever else breaks one of them keep the kernels above.  0: not built; A/B of a subset: DEFS=-DDTOF_HEADLINE_C2=0x6000
#ifndef DTOF_HEADLINE_C2
#define DTOF_HEADLINE_C2 0x3e000
#endif
constexpr uint32_t kHeadlineC2Facts = (DTOF_HEADLINE_C2) != 0 && kHeadlineFusedFacts != 0 ? (kHeadlineFusedFacts | (DTOF_HEADLINE_C2)) : 0u;
static_assert(((DTOF_HEADLINE_C2) & ~kFactsSampling) == 0, "DTOF_HEADLINE_C2 names route facts only (bits 13 and up)");
// ... and a fourth, tried first of all, with the shape of cornell_wall's flat table on top of that (i): DTOF_HEADLINE_SHAPE_COUNT rectangles, the wall at index
// DTOF_HEADLINE_SHAPE_WALL.  A one-wall room of any other shape takes the kernel above.  A/B without it: DEFS=-DDTOF_HEADLINE_SHAPE_COUNT=0
#ifndef DTOF_HEADLINE_SHAPE_COUNT
#define DTOF_HEADLINE_SHAPE_COUNT 5
#endif
#ifndef DTOF_HEADLINE_SHAPE_WALL
#define DTOF_HEADLINE_SHAPE_WALL 2
#endif
constexpr uint32_t kHeadlineShapeFacts = (DTOF_HEADLINE_SHAPE_COUNT) != 0 && (kHeadlineC2Facts & kFactOneWall) != 0 ? (kHeadlineC2Facts | flat_shape_fact(DTOF_HEADLINE_SHAPE_COUNT, DTOF_HEADLINE_SHAPE_WALL)) : 0u;
static_assert((DTOF_HEADLINE_SHAPE_COUNT) == 0 || (kHeadlineC2Facts & kFactOneWall) == 0 || (kHeadlineShapeFacts & kFactFlatShape) != 0, "a shape has 1 .. 8 objects and the wall among them");
// ... and a fifth, tried before all of them, with kFactPairSamples on top of that (j): C2's frame at its max_depth of 4.  The fact stands in front of two steps, each with
// a switch for its A/B.  DTOF_STREAM_JUMPS: the draws of the path stream whose values this kernel never reads (the emitter pick's two, the lobe pick's, the roulette's)
// advance the stream by pcg_jump<N> instead of one multiply-add each.  DTOF_PAIR_SAMPLES: each lane of a pair evaluates the BSDF direction of ONE sampling iteration
// (the even lane iteration 0's, the odd lane iteration 1's) right after generate_lane and the two exchange them; the bounce loop then holds no PCG arithmetic and no
// cosine_hemisphere.  Both 0: the text of kHeadlineShapeFacts under the new mask.  A/B without the instantiation: DEFS=-DDTOF_HEADLINE_PAIR=0
#ifndef DTOF_HEADLINE_PAIR
#define DTOF_HEADLINE_PAIR 1
#endif
#ifndef DTOF_STREAM_JUMPS
#define DTOF_STREAM_JUMPS 1
#endif
#ifndef DTOF_PAIR_SAMPLES
#define DTOF_PAIR_SAMPLES 1
#endif
constexpr uint32_t kHeadlinePairFacts = DTOF_HEADLINE_PAIR && kHeadlineShapeFacts != 0 ? (kHeadlineShapeFacts | kFactPairSamples) : 0u;
// ... and one more step behind the same fact (k).  DTOF_PAIR_WALK_PRIMARY: the camera ray, which is the same ray in the two lanes of a pair, splits its plain
// rectangles between the lanes (trace_flat's PAIR_RAYS form, dtof_pair_walk.h; written for a table of 5 with the wall at 2, every other shape keeps its text).
// The builds with the traversal counters compile the form out: a lane of it tests three rectangles, and the counters' slots 20 .. 23 count five.
// (The same form for iteration 0's shadow and continuation rays, in the waves whose primary hits are all off the wall, was built behind a switch of its own and
//  made the frame slower, alone and on top of this step: DESIGN 8.3 (k), profiles/pair_walk_ab.txt.  Removed.)
#ifndef DTOF_PAIR_WALK_PRIMARY
#define DTOF_PAIR_WALK_PRIMARY 1
#endif
// ... and another (l).  DTOF_PAIR_SETUP: what generate_lane computes for the PAIR -- the path stream's seeding, its two jitter draws, the sample position, the camera
// ray -- is evaluated once per pair instead of once per lane.  A block walks the chunks of its segment in sequence; at every even chunk lane L sets up pair L >> 1 of
// this chunk (L even) or of the next (L odd), the results stay in registers across the two chunks, and every lane of a chunk fetches its pair's from the lane that
// holds them (dtof_pair_setup.h).  0: generate_lane per lane, the parent's text.  DTOF_PAIR_SETUP_BPERMUTE: the fetch by ds_bpermute_b32, one text for both
// chunks; 0 (A/B): by DPP moves, quad_perm [0, 0, 2, 2] / [1, 1, 3, 3] behind a wave-uniform branch -- measured slower (profiles/pair_setup_ab.txt).
#ifndef DTOF_PAIR_SETUP
#define DTOF_PAIR_SETUP 1
#endif
#ifndef DTOF_PAIR_SETUP_BPERMUTE
#define DTOF_PAIR_SETUP_BPERMUTE 1
#endif
// the facts under which a lane's generation splits into a pair's piece and a lane's (dtof_sampling.h: generate_pair_part, generate_lane_part): one pass, the Doppler
// integrator's correlated sampler with every jitter draw from the path stream, stratified pairs, whole waves of one pixel
constexpr uint32_t kFactsLaneSplit = kFactSinglePass | kFactDopplerCorr | kFactCorrelated | kFactStratifiedPairs | kFactWavePixel;
constexpr bool lane_split_facts(uint32_t facts) { return (facts & kFactsLaneSplit) == kFactsLaneSplit; }
#ifdef DTOF_TRAVERSAL_STATS
constexpr bool kPairWalkCompiled = false;
#else
constexpr bool kPairWalkCompiled = true;
#endif
constexpr bool pair_walk_shape(uint32_t facts) { return (facts & kFactOneWall) != 0 && flat_shape_count(facts) == 5 && flat_shape_wall(facts) == 2; }
// The two steps of (i) inside trace_flat under a shape, each with a switch for its A/B: the occlusion queries' straight-line sweep, the closest-hit queries' written-out walk
#ifndef DTOF_FLAT_SHAPE_ANY
#define DTOF_FLAT_SHAPE_ANY 1
#endif
#ifndef DTOF_FLAT_SHAPE_CLOSEST
#define DTOF_FLAT_SHAPE_CLOSEST 1
#endif
// DTOF_WALL_FRAMES (default 1): under kFactOneWall the shading frames come precomputed -- the plain rectangles' from the DFlatFrame table of the blob, the moving wall's
// normal and tangent from two registers filled once per path (k_shade) -- so that compute_surface runs no normalisation.  0 builds the facts without them (A/B).
#ifndef DTOF_WALL_FRAMES
#define DTOF_WALL_FRAMES 1
#endif
// ... and the resident Domino kernel of one film at 16 waves (dtof_shade_res0.hip): every fact but kFactOneBlock, which describes the classic launch (0: not built)
#ifndef DTOF_RESIDENT_FACTS
#define DTOF_RESIDENT_FACTS 0x37f
#endif
constexpr uint32_t kResidentFacts = DTOF_RESIDENT_FACTS;

// One launch of k_shade as launch_shade hands it to the translation unit that holds the instantiation (dtof_shade_*.hip: the ~100 instantiations of the
// kernel compile in parallel, one group per file): staged = the scene blob is copied to LDS by every block; mode 0 split, 1 fused, 2 fused first bounce;
// waves != 0: the resident form (`waves` waves per block, one block per CU); lds: the launch's dynamic LDS (ShadeLds::bytes), lds_flat: the same without the stack columns, what a kernel compiled
// with kFactFlat is launched with; facts: the plan facts this launch satisfies (0: take the generic kernels).  launch_shade_plain and launch_shade_resident0 return the mask of the instantiation specialised on plan facts that ran, 0 if a generic one did.
struct ShadeLaunch { bool staged; int mode; uint32_t waves, grid, lds, lds_flat; hipStream_t stream; ShadeArgs args; uint32_t facts; };
uint32_t launch_shade_plain(bool area, bool k4, const ShadeLaunch &L);  // rectangle-only diffuse scenes          (dtof_shade_plain.hip)
void launch_shade_mesh(bool area, bool k4, const ShadeLaunch &L);       // + triangles / analytic shapes          (dtof_shade_mesh.hip)
void launch_shade_spec1(bool k4, const ShadeLaunch &L);                 // every BSDF / emitter / texture         (dtof_shade_spec1.hip)
void launch_shade_spec2(bool k4, const ShadeLaunch &L);                 // ... and blendbsdf                      (dtof_shade_spec2.hip)
uint32_t launch_shade_resident0(bool area, bool k4, const ShadeLaunch &L);  // resident first bounce, diffuse scenes  (dtof_shade_res0.hip)
void launch_shade_resident1(bool k4, const ShadeLaunch &L);             // resident first bounce, every BSDF      (dtof_shade_res1.hip)
void launch_shade_resident2(bool k4, const ShadeLaunch &L);             // ... and blendbsdf                      (dtof_shade_res2.hip)

// Resident stage of the fused first-bounce kernel (k_shade<..., RESW>, dtof_kernels.hip): `waves` waves per block (0 = off), one block per CU of the n_cu the
// device has; the block [small_off, small_off + 16 * small_words) of the blob (groups, shapes, emitters, triangles, shading data) and the TLAS nodes live in LDS.
struct ResidentStage { uint32_t small_off = 0, small_words = 0, waves = 0, n_cu = 0; };
inline ShadeLds resident_lds(const RenderParams &rp, const ResidentStage &st, uint32_t stack_depth, uint32_t waves) { return ShadeLds::resident(st.small_words, waves, rp.memo_obj != 0xffffffffu, rp.n_offsets != 1, stack_depth); }
uint32_t device_lds_limit();   // asked once per frame (plan_frame): hipDeviceAttributeMaxSharedMemoryPerBlock of the current device (160 KiB on gfx950), minus the kernels' static LDS
uint32_t device_cu_count();    // ... and hipDeviceAttributeMultiprocessorCount

// The launchers' development switches, read once per frame with the others (dtof_render.hip: plan_frame, which lists them)
struct LaunchSwitches {
    int defer = 2;                              // DTOF_DEFER: ray kernels as a pair of launches (0 when the frame's workspace has no DEFER lists)
    bool trace8 = true, nodes16 = true, tlas_lds = true, stage = true;   // DTOF_TRACE8 / NODES16 / TLAS_LDS / STAGE
    bool xcd_set = false; uint32_t xcd_remap = 0;                          // DTOF_XCD_REMAP, when set
    uint32_t trace_block = 0;                   // DTOF_TRACE_BLOCK: 64 / 128 / 256, 0 = automatic
    int splat = 0;                              // DTOF_SPLAT: 0 automatic, 1 dpp, 2 generic
};

// kernels (dtof_kernels.hip)
void launch_generate(const RenderParams &rp, const Queues &q, hipStream_t s);
void launch_sum_counts(const uint32_t *counts, uint32_t n_seg, uint32_t n_rows, unsigned long long *out, hipStream_t s);
uint32_t segments_for(uint32_t n_lanes);   // number of queue segments (count slots) for a batch
void launch_trace(const uint8_t *scene, uint32_t scene_bytes, const RenderParams &rp, const Queues &q,
                  const uint32_t *qin, const uint32_t *count_in, uint32_t stack_depth, const LaunchSwitches &ls, hipStream_t s);
// One launch of k_shade as render_rows asks for it
struct ShadeRequest {
    const uint8_t *scene = nullptr; uint32_t scene_bytes = 0, stack_depth = 0;   // the blob on the device; stack entries a traversal of it can need
    const RenderParams *rp = nullptr; const Queues *q = nullptr; const LaunchSwitches *switches = nullptr; hipStream_t stream = nullptr;
    const uint32_t *qin = nullptr, *count_in = nullptr;                       // the lane queue and segment counts it reads (nullptr: every lane of the batch)
    uint32_t *qout = nullptr, *alive_out = nullptr, *shadow_out = nullptr;    // the lane queue it writes; the count slots of its last iteration
    uint32_t depth = 0; int mode = 0; bool trace_next = false;                // its first iteration; 0 split, 1 fused, 2 fused first bounce (generate + primary trace inline); an iteration follows
    LaneDebug *dbg = nullptr; float *film = nullptr; uint64_t film_stride = 0;   // first bounce of a lane dump: the camera rays; film: the launch covers the whole path and splats its lanes itself
    uint32_t facts = 0; const ResidentStage *resident = nullptr;              // the plan facts it satisfies (kFact*); the plan made it a resident launch (LaunchSpan::resident) of this stage
};
uint32_t launch_shade(const ShadeRequest &r);   // returns the FACTS mask of the kernel that ran (0: a generic one)
void launch_shadow(const uint8_t *scene, uint32_t scene_bytes, const RenderParams &rp, const Queues &q,
                   const uint32_t *count_in, uint32_t stack_depth, const LaunchSwitches &ls, hipStream_t s);
void launch_velocity(const uint8_t *scene, uint32_t scene_bytes, const RenderParams &rp, const Queues &q, uint32_t stack_depth, const LaunchSwitches &ls, hipStream_t s);
// returns the packed choice of the kernel it launched (dtof_splat_choice.h: SplatChoice::packed), 0 for an empty batch
uint32_t launch_splat(const RenderParams &rp, const Queues &q, float *film, uint64_t plane_stride, const LaunchSwitches &ls, hipStream_t s);
void launch_lane_dump(const RenderParams &rp, const Queues &q, LaneDebug *out, hipStream_t s);
void launch_pass_save(const RenderParams &rp, const Queues &q, hipStream_t s);   // multi-pass: main / path stream states of the batch -> rp.pass_rng
void launch_lane_dump_rays(const RenderParams &rp, const Queues &q, LaneDebug *out, hipStream_t s);

// sampler KAT kernels
struct SamplerState { uint2 *rng, *rng_time, *rng_path; uint32_t *perm_seed, *dim; uint32_t n; };
void launch_sampler_seed(const RenderParams &rp, const SamplerState &st, hipStream_t s);
void launch_sampler_next_correlate(const RenderParams &rp, const SamplerState &st, const uint8_t *correlate, int correlate_all,
                                   float *out, hipStream_t s);
void launch_sampler_next_1d(const RenderParams &rp, const SamplerState &st, float *out, hipStream_t s);
void launch_sampler_next_time(const RenderParams &rp, const SamplerState &st, uint32_t sample_index_base, float *out, hipStream_t s);
void launch_waveform_eval(const RenderParams &rp, const float *t, const float *len, float *out, int mode, uint32_t n, hipStream_t s);

// component evaluation (dtof_eval_component; the ids are the DTOF_COMP_* values of include/dtof.h)
enum { COMP_MICROFACET_EVAL = 0, COMP_MICROFACET_PDF = 1, COMP_MICROFACET_G1 = 2, COMP_MICROFACET_SAMPLE = 3, COMP_FRESNEL = 4,
       COMP_FRESNEL_CONDUCTOR = 5, COMP_RFILTER = 6, COMP_WARP_COSINE_HEMISPHERE = 7, COMP_WARP_DISK_CONCENTRIC = 8,
       COMP_WARP_UNIFORM_TRIANGLE = 9, COMP_WARP_UNIFORM_SPHERE = 10, COMP_COORDINATE_SYSTEM = 11, COMP_TEA_FLOAT32 = 12, COMP_MATH = 13,
       COMP_COUNT = 14 };
struct ComponentArgs { int component; float p[8]; const float *in; int in_stride; float *out; int out_stride; uint32_t n; };
void launch_component(const ComponentArgs &a, const RenderParams &rp, hipStream_t s);
// BSDF::eval_pdf_sample over arrays, one launcher per SPEC instantiation of bsdf_eval_pdf_sample, each in the file that holds that SPEC's shade kernels
// (dtof_shade_plain.hip, dtof_shade_spec1.hip, dtof_shade_spec2.hip); in: 29 floats per query, out: 14 (k_bsdf_eval, dtof_shade.h)
void launch_bsdf_eval_0(const uint8_t *scene, uint32_t shape_index, const float *in, float *out, uint32_t n, hipStream_t s);
void launch_bsdf_eval_1(const uint8_t *scene, uint32_t shape_index, const float *in, float *out, uint32_t n, hipStream_t s);
void launch_bsdf_eval_2(const uint8_t *scene, uint32_t shape_index, const float *in, float *out, uint32_t n, hipStream_t s);
// The emitter side of a path vertex over arrays (dtof_emitter_eval; k_emitter_eval, dtof_shade.h), one launcher per file of shade kernels for the (AREA, MESH, SPEC)
// levels of that file: 0 (F,F,0), 1 (T,F,0) and 6 (level 0 under kFactOneEmitter) plain; 2 (F,T,0), 3 (T,T,0) mesh; 4 (T,T,1) spec1; 5 (T,T,2) spec2
void launch_emitter_eval_plain(const uint8_t *scene, int level, int mode, uint32_t index, float pmf, const float *in, float *out, uint32_t n, hipStream_t s);
void launch_emitter_eval_mesh(const uint8_t *scene, int level, int mode, uint32_t index, float pmf, const float *in, float *out, uint32_t n, hipStream_t s);
void launch_emitter_eval_spec1(const uint8_t *scene, int level, int mode, uint32_t index, float pmf, const float *in, float *out, uint32_t n, hipStream_t s);
void launch_emitter_eval_spec2(const uint8_t *scene, int level, int mode, uint32_t index, float pmf, const float *in, float *out, uint32_t n, hipStream_t s);
void launch_camera_rays(const RenderParams &rp, const float *in, float *out, uint32_t n, hipStream_t s);   // Sensor::sample_ray over arrays (known-answer entry)
// The eight-wave ray kernels (k_trace / k_shadow<..., W8>, dtof_kernels.hip): LDS entries of a lane's traversal stack and entries of its private overflow array; the
// largest TLAS they copy into LDS (nodes)
constexpr uint32_t kLdsStack8 = 16, kOvfStack8 = 48, kTlasLds8 = 16;
// Scene::ray_intersect / ray_test over arrays
void launch_ray_query(const uint8_t *scene, const float *rays, float *out, int32_t *ids, float *uv4, uint32_t n, bool any, uint32_t stack_depth, hipStream_t s);

#ifdef DTOF_TRAVERSAL_STATS
constexpr uint32_t kTravStats = 24;   // counter slots (dtof_traverse.h)
bool read_traversal_stats(unsigned long long *out8);   // all kTravStats slots
void register_traversal_stats_reader(bool (*reader)(unsigned long long *acc8));
#endif

}  // namespace dtof
