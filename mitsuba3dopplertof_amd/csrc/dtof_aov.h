// dtof_aov.h -- launcher of the geometry channels of the reference's `aov` integrator (src/integrators/aov.cpp:196-330: the camera ray is intersected once and the
// fields of the surface interaction become channels that ImageBlock::put filters like the image, src/render/imageblock.cpp:414-531).  k_aov (dtof_aov.hip) takes the
// place of the shade loop behind k_generate: one closest hit per lane at the ray's own time, the surface interaction with its frames, and the splat into a film of
// doubles -- or, for the per-lane entry, the lane's values written out instead of the splat.  Only the host orchestration reads this header.
//
// A lane has kAovSlots = 20 VALUES, all of them +0 on a miss (aov.cpp:208 zeroes the interaction):
//   0            si.t                                      depth        (aov.cpp:247-249)
//   1 .. 3       si.p                                      position     (:251-255)
//   4, 5         si.uv                                     uv           (:257-260)
//   6 .. 8       si.n                                      geo_normal   (:262-266)
//   9 .. 11      si.sh_frame.n                             sh_normal    (:268-272)
//   12 .. 14     si.dp_du                                  dp_du        (:278-282)
//   15 .. 17     si.dp_dv                                  dp_dv        (:284-288)
//   18           (float) si.prim_index                     prim_index   (:300-302)
//   19           (float) (1 + index of the shape record)   shape_index  (:304-306; the numbering: include/dtof.h)
// CHANNEL c of a film or of a lane's output row is value slot[c]: the table follows the order of the spec, a type may occur several times.
// FILM: the cells of dtof_moments.h -- kMomentCell = 32 doubles per pixel, cell[0] the sum of the weights, cell[1 + c] channel c, so at most kAovMaxChannels = 31
// channels.  Terms are formed like the moment film's: value * (wx * wy) a float32 product (the box filter adds the value itself and 1), converted to double, and only
// double additions from there on.  launch_develop_moments turns the cells into the dense planes the C ABI hands out.
#pragma once
#include "dtof_kernels.h"
#include "dtof_moments.h"

namespace dtof {

constexpr int kAovSlots = 20, kAovMaxChannels = kMomentCell - 1;
constexpr int kAovTypes = 9;
constexpr uint32_t kAovSlotsPerWord = 12;
// first slot and channel count of type t (the DTOF_AOV_* constants of include/dtof.h, in their order)
constexpr int kAovTypeSlot[kAovTypes] = { 0, 1, 4, 6, 9, 12, 15, 18, 19 }, kAovTypeChannels[kAovTypes] = { 1, 3, 2, 3, 3, 3, 3, 1, 1 };

// The FLOW film (dtof_render_flow, dtof_sample_flow_lanes; the definition: include/dtof.h) is the same kernel compiled with two more values per lane, the motion
// vector of the camera ray's hit over the shutter interval:
//   20, 21       flow x, y                                 (no counterpart in the reference's aov integrator: the nine types above are not extended)
// Only a request with AovArgs::flow set reaches those instantiations; its private channel table is (20, 21).
constexpr int kAovFlowSlots = kAovSlots + 2;

struct AovArgs {
    double *film;            // cells of kMomentCell doubles per pixel of the crop window, or
    float *values;           // ... nullptr, or [n_lanes][n_channels]: the values of the batch's lanes instead of the splat
    uint32_t n_channels;     // 1 .. kAovMaxChannels
    uint64_t slots[3];       // slot[c] = the 5 bits from bit 5 * (c % kAovSlotsPerWord) of word c / kAovSlotsPerWord
    uint32_t flow;           // 1: the FLOW instantiations, whose lanes have the values 20 and 21; S is read only then
    double S[12];            // world to film pixel, rows x, y, w (dtof_world_to_pixel.h)
};

// One batch behind k_generate: q.ray_a / ray_b / pos of lanes [0, rp.n_lanes).  Stages the scene like launch_velocity.
void launch_aov(const uint8_t *scene, uint32_t scene_bytes, const RenderParams &rp, const Queues &q, const AovArgs &a, uint32_t stack_depth, const LaunchSwitches &ls,
                hipStream_t s);

}  // namespace dtof
