#pragma once
// dtof_traverse.h -- device side of the scene: blob view, LDS staging, primitive tests (rectangle, triangle, sphere), motion-blur
// instance matrices and the TLAS / BLAS traversal (closest hit and occlusion).  Included by dtof_kernels.hip only.
#include "dtof_kernels.h"
#include "dtof_scene.h"
#include "dtof_math.h"
#include "dtof_flat_cull.h"
#include "dtof_box_cull.h"
#include "dtof_pair_walk.h"
#include "dtof_zrow_mfma.h"

#ifndef DTOF_D
#define DTOF_D __device__ __forceinline__
#endif

namespace dtof {

// ---------------------------------------------------------------------------- scene view
struct SceneView {
    const DNode *nodes; const DNode16 *nodes16; const DObject *objects; const DGroup *groups; const DShape *shapes;
    const DTri *tris; const DTriIsect *isect; const DTriShade *shading; const DEmitter *emitters; const uint8_t *base;
    uint32_t n_nodes, n_emitters;
    // Fused shade kernels, scenes with ONE instance object: the world -> object matrix of that instance at the lane's ray time is
    // computed once per path vertex (instance_memo_fill) and kept in a per-thread LDS column; the closest-hit and occlusion queries of
    // the vertex and its surface interaction read it back instead of re-deriving it (a ray's time does not change along a path,
    // dopplertofpath.cpp:93,240-244).  memo_obj = 0xffffffff: no memo.
    uint32_t memo_obj; float *memo;
    bool memo_m;   // the column also holds the instance matrix itself (words 12 .. 23; the flat scenes' kernels, whose LDS has the room): compute_surface reads both back
};
// Resident scene stage (k_shade<..., RESW>): the TLAS nodes live in LDS as FOUR PLANES of 16-byte pieces -- piece k of node i at
// uint4 index k * kResNodes + i -- so that the 16 lanes of a ds_read_b128 lane group, which read the same piece of 16 different nodes,
// spread over all 64 banks (node-major 64-byte records would put piece k of every node on the same 16 banks: 4-way conflicts on
// average); the plane stride is a compile-time constant, so the four reads of a node step are one address plus immediate offsets.
constexpr uint32_t kResNodes = 1024;
// ... and in the kernels of SEVERAL films their child references are re-encoded to 16 bits while they are copied (at most 1 024 nodes, and a TLAS of that size has at
// most 1 025 objects): leaf flag = bit 15, "no child" = 0xffff.  The traversal stack of those kernels then holds 16-BIT entries -- half the LDS of the 32-bit columns
// (Domino: 24 instead of 48 KiB at 16 waves), which pays for the film-state AND the path-state columns of k_shade (round 5: C5 164.9 -> 156.4 ms).  The one-film kernels
// keep 32-bit entries: their columns fit as they are, and the 16-bit form costs them 0.8 % (C4 33.74 -> 34.02 ms; profiles/r05_k4_film_state.txt).
constexpr uint32_t kLeafFlag16 = 0x8000u, kNoChild16 = 0xffffu, kDone16 = 0x7fffu;
DTOF_D uint32_t encode_child16(uint32_t w) { return w == kNoChild ? kNoChild16 : ((w & 0x7fffu) | ((w >> 16) & 0x8000u)); }
DTOF_D SceneView make_view(const uint8_t *base) {
    const BlobHeader *h = (const BlobHeader *) base;
    SceneView v;
    v.nodes = (const DNode *) (base + h->off_nodes);
    v.nodes16 = (const DNode16 *) (base + h->off_nodes16);   // (meaningful where off_nodes16 != 0: the launch picks the kernels that read it)
    v.objects = (const DObject *) (base + h->off_objects);
    v.groups = (const DGroup *) (base + h->off_groups);
    v.shapes = (const DShape *) (base + h->off_shapes);
    v.tris = (const DTri *) (base + h->off_tris);
    v.isect = (const DTriIsect *) (base + h->off_isect);
    v.shading = (const DTriShade *) (base + h->off_shading);
    v.emitters = (const DEmitter *) (base + h->off_emitters);
    v.base = base;
    v.n_nodes = h->n_nodes; v.n_emitters = h->n_emitters;
    v.memo_obj = 0xffffffffu; v.memo = nullptr; v.memo_m = false;
    return v;
}
// Stage the whole scene blob into LDS (small scenes: the Cornell blob is ~5 KB).
DTOF_D const uint8_t *stage_scene(const uint8_t *g, uint32_t bytes, uint4 *lds) {
    const uint4 *src = (const uint4 *) g;
    for (uint32_t i = threadIdx.x; i < bytes / 16; i += blockDim.x) lds[i] = src[i];
    __syncthreads();
    return (const uint8_t *) lds;
}

struct Hit { float t, u, v; uint32_t obj, shape, prim; };

// Traversal statistics (development builds only: make STATS=1 -> libdtof_stats.so, read by tools/traversal_stats.py).
// [0] rays  [1] node steps (lane)  [2] node iterations (wave)  [3] leaf visits (lane)  [4] leaf rounds (wave)  [5] mesh loops entered (lane)
// [6] triangle tests (lane)  [7] BLAS node steps (lane)  [8] instance transforms (lane)  [9] instance transforms (wave)  [10] mesh loops entered (wave)
// [11] triangle tests (wave)  [12] rectangle tests (lane)  [13] rectangle tests (wave)
// [14] POISON HITS: in these builds k_shade gives the path state of every lane that has no path (beyond the end of its segment) a recognisable pattern (kPoisonState) and
//      counts it wherever path state leaves the registers -- queue stores, the LDS columns, the inline iterations' hand-over.  Must stay 0: the K = 4 incident of round 3
//      (profiles/r03_k4_uninitialised.txt, profiles/r05_k4_root_cause.txt) was a film that depended on the INITIAL value of those registers.
// [15] BLAS node steps (wave)
// [16 .. 19] trace_flat, occlusion rays: rectangles whose z row was tested (lane), ... that it settled as certain misses (lane), z-row tests (wave), full tests (wave:
//      the waves in which some lane still needed it);  [20 .. 23] the same for closest-hit rays.  dtof_debug_traversal_stats reads slots 0 .. 15, dtof_debug_traversal_stats_n all.
#ifdef DTOF_TRAVERSAL_STATS
// every translation unit with kernels counts into its own copy (no relocatable device code); each registers a reader, read_traversal_stats sums and resets them all
static __device__ unsigned long long g_trav_stats[kTravStats];
static bool read_tu_traversal_stats(unsigned long long *acc8) {
    unsigned long long v[kTravStats], zero[kTravStats] = { 0 };
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_trav_stats), sizeof v) != hipSuccess || hipMemcpyToSymbol(HIP_SYMBOL(g_trav_stats), zero, sizeof zero) != hipSuccess) return false;
    for (uint32_t i = 0; i < kTravStats; ++i) acc8[i] += v[i];
    return true;
}
static const int g_trav_stats_registered = (register_traversal_stats_reader(read_tu_traversal_stats), 0);
#define DTOF_STAT(i) atomicAdd(&g_trav_stats[i], 1ull)
#define DTOF_STAT_WAVE(i) do { if (__lane_id() == (uint32_t) __ffsll((long long) __ballot(1)) - 1u) atomicAdd(&g_trav_stats[i], 1ull); } while (0)
#else
#define DTOF_STAT(i) ((void) 0)
#define DTOF_STAT_WAVE(i) ((void) 0)
#endif

// What a query REPORTS as a hit's primitive: Hit::prim addresses the scene's triangle arrays, which a mesh's BLAS build permutes (compute_surface reads them through
// it); PreliminaryIntersection::prim_index is the face in the mesh's own order.  The primitive of any other shape is reported as it is.
DTOF_D uint32_t hit_prim_index(const SceneView &sv, const Hit &h) {
    const DObject &ob = sv.objects[h.obj];
    const DShape &sh = sv.shapes[(ob.kind == OBJ_INSTANCE ? sv.groups[ob.index].first_shape : ob.index) + h.shape];
    return sh.kind == SHAPE_MESH ? sv.tris[sh.first_tri + h.prim].face : h.prim;
}

// ---------------------------------------------------------------------------- primitives
// Rectangle::ray_intersect_preliminary_impl, src/shapes/rectangle.cpp:201-224
DTOF_D bool rect_hit(const DShape &sh, V3 o, V3 d, float maxt, float &t, float &u, float &v) {
    V3 lo = xf_point(sh.to_object, o), ld = xf_vector(sh.to_object, d);
    t = -lo.z / ld.z;
    u = fmaf(ld.x, t, lo.x); v = fmaf(ld.y, t, lo.y);
    return t >= 0.f && t <= maxt && fabsf(u) <= 1.f && fabsf(v) <= 1.f;
}
// Disk::ray_intersect_preliminary_impl, src/shapes/disk.cpp:216-232: the rectangle's plane test with a circular bound
DTOF_D bool disk_hit(const DShape &sh, V3 o, V3 d, float maxt, float &t, float &u, float &v) {
    V3 lo = xf_point(sh.to_object, o), ld = xf_vector(sh.to_object, d);
    t = -lo.z / ld.z;
    u = fmaf(ld.x, t, lo.x); v = fmaf(ld.y, t, lo.y);
    return t >= 0.f && t <= maxt && u * u + v * v <= 1.f;
}
// Moeller-Trumbore as in Embree 3's triangle intersector (tnear < t <= tfar; u,v weight vertices 1,2).  The 48-byte record (DTriIsect: first vertex, edges and
// geometric normal, precomputed on the host with these operations) is fetched with three 16-byte loads issued together.
DTOF_D bool tri_hit(const DTriIsect &tr, V3 o, V3 d, float maxt, float &t, float &u, float &v) {
    const uint4 *tp = (const uint4 *) &tr;
    const uint4 q0 = tp[0], q1 = tp[1], q2 = tp[2];
    const V3 p0 = mk(u2f(q0.x), u2f(q0.y), u2f(q0.z)), e1 = mk(u2f(q1.x), u2f(q1.y), u2f(q1.z)), e2 = mk(u2f(q2.x), u2f(q2.y), u2f(q2.z));
    const V3 ng = mk(u2f(q0.w), u2f(q1.w), u2f(q2.w));
    V3 c = p0 - o, r = cross(c, d);
    float den = dot(ng, d), aden = fabsf(den);
    uint32_t sgn = f2u(den) & 0x80000000u;
    float U = u2f(f2u(dot(r, e2)) ^ sgn), Vv = u2f(f2u(dot(r, e1)) ^ sgn);
    if (!(den != 0.f && U >= 0.f && Vv >= 0.f && U + Vv <= aden)) return false;
    float T = u2f(f2u(dot(ng, c)) ^ sgn);
    if (!(0.f < T && T <= aden * maxt)) return false;
    float rc = 1.0f / aden;
    u = U * rc; v = Vv * rc; t = T * rc;
    return true;
}
// math::solve_quadratic (include/mitsuba/core/math.h:357-401), float64
DTOF_D bool solve_quadratic_d(double a, double b, double c, double &x0, double &x1) {
    const bool linear = a == 0.0, valid_linear = linear && b != 0.0;
    x0 = x1 = -c / b;
    const double discrim = fma(b, b, -(4.0 * a * c));
    const bool valid_quadratic = !linear && discrim >= 0.0;
    if (valid_quadratic) {
        const double sq = sqrt(discrim), temp = -0.5 * (b + copysign(sq, b));
        const double x0p = temp / a, x1p = c / temp;
        x0 = x0p < x1p ? x0p : x1p; x1 = x0p < x1p ? x1p : x0p;
    }
    return valid_linear || valid_quadratic;
}
DTOF_D double dot3d(double ax, double ay, double az, double bx, double by, double bz) { return fma(az, bz, fma(ay, by, ax * bx)); }
// Sphere::ray_intersect_preliminary_impl (src/shapes/sphere.cpp:338-394) / ray_test_impl (:396-431): float64 on the llvm back
// end; the point of the ray closest to the centre is evaluated with the FLOAT ray (Ray::operator() takes a Float, ray.h:61).
template <bool ANY>
DTOF_D bool sphere_hit(const DShape &sh, V3 o, V3 d, float maxt_f, float &t_out) {
    const double radius = sh.dp_du[0], cx = sh.n[0], cy = sh.n[1], cz = sh.n[2], maxt = maxt_f;
    const double dx = d.x, dy = d.y, dz = d.z;
    double near_t, far_t;
    if (ANY) {
        const double ox = (double) o.x - cx, oy = (double) o.y - cy, oz = (double) o.z - cz;
        const double A = dot3d(dx, dy, dz, dx, dy, dz), B = 2.0 * dot3d(ox, oy, oz, dx, dy, dz), C = dot3d(ox, oy, oz, ox, oy, oz) - radius * radius;
        const bool found = solve_quadratic_d(A, B, C, near_t, far_t);
        const bool out_bounds = !(near_t <= maxt && far_t >= 0.0), in_bounds = near_t < 0.0 && far_t > maxt;
        return found && !out_bounds && !in_bounds;
    }
    const double lx = (double) o.x - cx, ly = (double) o.y - cy, lz = (double) o.z - cz;
    const double plane_t = dot3d(-lx, -ly, -lz, dx, dy, dz) / sqrt(dot3d(dx, dy, dz, dx, dy, dz));
    bool no_hit = plane_t == 0.0 && (o.x != sh.n[0] && o.y != sh.n[1] && o.z != sh.n[2]);
    const V3 pp = vfma(d, (float) plane_t, o);
    const double ox = (double) pp.x - cx, oy = (double) pp.y - cy, oz = (double) pp.z - cz;
    no_hit = no_hit && sqrt(dot3d(ox, oy, oz, ox, oy, oz)) > radius;
    const double A = dot3d(dx, dy, dz, dx, dy, dz), B = 2.0 * dot3d(ox, oy, oz, dx, dy, dz), C = dot3d(ox, oy, oz, ox, oy, oz) - radius * radius;
    const bool found = solve_quadratic_d(A, B, C, near_t, far_t);
    near_t += plane_t; far_t += plane_t;
    const bool out_bounds = !(near_t <= maxt && far_t >= 0.0), in_bounds = near_t < 0.0 && far_t > maxt;
    if (!(found && !no_hit && !out_bounds && !in_bounds)) return false;
    t_out = near_t < 0.0 ? (float) far_t : (float) near_t;
    return true;
}
// Cylinder::ray_intersect_preliminary_impl / ray_test_impl (src/shapes/cylinder.cpp:300-391): the unit cylinder in object space, float64 on the
// llvm back end (the ray is transformed in float32, then widened)
DTOF_D bool cylinder_hit(const DShape &sh, V3 o, V3 d, float maxt_f, float &t_out) {
    const V3 lo = xf_point(sh.to_object, o), ld = xf_vector(sh.to_object, d);
    const double ox = lo.x, oy = lo.y, oz = lo.z, dx = ld.x, dy = ld.y, dz = ld.z, maxt = maxt_f;
    const double A = dx * dx + dy * dy, B = 2.0 * (dx * ox + dy * oy), C = ox * ox + oy * oy - 1.0;
    double near_t, far_t;
    const bool found = solve_quadratic_d(A, B, C, near_t, far_t);
    const bool out_bounds = !(near_t <= maxt && far_t >= 0.0), in_bounds = near_t < 0.0 && far_t > maxt;
    const double z_near = oz + dz * near_t, z_far = oz + dz * far_t;
    const bool near_ok = z_near >= 0.0 && z_near <= 1.0 && near_t >= 0.0, far_ok = z_far >= 0.0 && z_far <= 1.0 && far_t <= maxt;
    if (!(found && !out_bounds && !in_bounds && (near_ok || far_ok))) return false;
    t_out = near_ok ? (float) near_t : (float) far_t;
    return true;
}
// AnimatedTransform::eval, include/mitsuba/core/transform.h:439-466
DTOF_D void instance_matrix(const DObject &ob, float time, float *m) {
    if (ob.n_keys <= 1) {
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = ob.key0[i];
        return;
    }
    float t = fmin_(fmax_((time - ob.t0) / (ob.t1 - ob.t0), 0.f), 1.f), omt = 1 - t;
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = ob.key0[i] * omt + ob.key1[i] * t;
}

// instance memo (see SceneView): kMemoWords words per thread, word k of thread t at memo[k * kMemoStride + t] (dtof_kernels.h)
DTOF_D void instance_memo_fill(const SceneView &sv, float time, float *m, float *inv) {
    instance_matrix(sv.objects[sv.memo_obj], time, m);
    affine_inverse(m, inv);
#pragma unroll
    for (uint32_t k = 0; k < kMemoWords; ++k) sv.memo[k * kMemoStride] = inv[k];
    if (sv.memo_m) {
#pragma unroll
        for (uint32_t k = 0; k < kMemoWords; ++k) sv.memo[(kMemoWords + k) * kMemoStride] = m[k];
    }
}
DTOF_D void instance_memo_load_matrix(const SceneView &sv, float *m) {   // only where sv.memo_m
#pragma unroll
    for (uint32_t k = 0; k < kMemoWords; ++k) m[k] = sv.memo[(kMemoWords + k) * kMemoStride];
}
DTOF_D void instance_memo_load(const SceneView &sv, float *inv) {
#pragma unroll
    for (uint32_t k = 0; k < kMemoWords; ++k) inv[k] = sv.memo[k * kMemoStride];
}

// Slab test of a padded box: dtof_box_cull.h (slab_ray, box_hit; a header a host program can compile) has the functions, their contract -- the test only culls, and
// never a box the exact ray meets within [0, tbest] -- and the error bound behind it.
DTOF_D SlabRay slab_ray(V3 o, V3 d) { return slab_ray(o.x, o.y, o.z, d.x, d.y, d.z); }
// Traversal stack entry `sp` of this thread: a per-thread LDS column (32-bit, or 16-bit in the resident kernels of several films) -- and, in the eight-waves-per-SIMD
// ray kernels of large meshes (k_trace / k_shadow<..., W8>), only its first LDSN entries: deeper ones overflow into a private array `ovf` (scratch memory; a BLAS of half a
// million triangles is 20-odd levels deep, a traversal rarely holds more than a dozen entries), so that 32 one-wave blocks fit a CU's LDS instead of 23.
template <bool S16, uint32_t LDSN>
DTOF_D void stack_put(uint32_t *stack, uint32_t *ovf, int sp, uint32_t stride, uint32_t x) {
    // (LDSN: the empty asm keeps the two stores in their branches -- merged, they become ONE flat_store through a select of the scratch and the LDS address, and a flat
    //  access goes through the texture-address unit these kernels saturate; round 5, read in the ISA of k_trace<false, true, 64, true>)
    if (LDSN != 0 && (uint32_t) sp >= LDSN) { ovf[(uint32_t) sp - LDSN] = x; return; }
    if (S16) ((uint16_t *) stack)[sp * stride] = (uint16_t) x;
    else stack[sp * stride] = x;
    if (LDSN != 0) asm volatile("" : : "v"(x));   // BEHIND the store: the last instructions of the two branches differ, the stores are not sunk into one
}
template <bool S16, uint32_t LDSN>
DTOF_D uint32_t stack_get(const uint32_t *stack, const uint32_t *ovf, int sp, uint32_t stride) {
    if (LDSN != 0 && (uint32_t) sp >= LDSN) return ovf[(uint32_t) sp - LDSN];
    uint32_t x = S16 ? (uint32_t) ((const uint16_t *) stack)[sp * stride] : stack[sp * stride];
    if (LDSN != 0) asm volatile("" : "+v"(x));   // (see stack_put: a ds_read in its own branch, not a flat access)
    return x;
}
// One traversal step at inner node `cur` = four 16-byte loads issued together (no load depends on a field of the node): continue with the nearest child that is
// hit, push the other, pop when nothing is hit.  STRIDE: the stride of the per-thread stack columns when the kernel knows its block size (a shift instead of v_mul_lo_u32).
DTOF_D float half_lo(uint32_t w) { return (float) __builtin_bit_cast(_Float16, (uint16_t) (w & 0xffffu)); }
DTOF_D float half_hi(uint32_t w) { return (float) __builtin_bit_cast(_Float16, (uint16_t) (w >> 16)); }
template <bool SOA = false, uint32_t STRIDE = 0, bool S16 = false, uint32_t LDSN = 0, bool H16 = false>   // S16: 16-bit child references and stack entries (the resident kernels of several films); LDSN: LDS entries before the overflow; H16: `nodes` points at DNode16 records (half-float boxes: two loads)
DTOF_D uint32_t node_step(const BvhNode *nodes, uint32_t cur, const SlabRay &r, float tbest, uint32_t *stack, int &sp, int sp_floor, uint32_t stride_rt, uint32_t done, uint32_t *ovf = nullptr) {
    const uint32_t stride = STRIDE ? STRIDE : stride_rt;
    if (H16) {
        // (SOA: the resident stage's LDS copy -- TWO planes of 2 * kResNodes pieces, piece k of node i at k * 2 * kResNodes + i: 2 048 half-float nodes in the 64 KiB of 1 024 float ones)
        const uint4 *np = SOA ? (const uint4 *) nodes + cur : (const uint4 *) ((const DNode16 *) nodes + cur);
        const uint4 a = np[0], b = np[SOA ? 2 * kResNodes : 1];
        const float lmin[3] = { half_lo(a.x), half_hi(a.x), half_lo(a.y) }, lmax[3] = { half_hi(a.y), half_lo(a.z), half_hi(a.z) };
        const float rmin[3] = { half_lo(b.x), half_hi(b.x), half_lo(b.y) }, rmax[3] = { half_hi(b.y), half_lo(b.z), half_hi(b.z) };
        const uint32_t left = a.w, right = b.w;
        float tl, tr;
        const bool hl = box_hit(lmin, lmax, r, tbest, tl);
        const bool hr = (int) box_hit(rmin, rmax, r, tbest, tr) & (int) (right != (S16 ? kNoChild16 : kNoChild));
        if (hl && hr) {
            const bool left_first = tl <= tr;
            stack_put<S16, LDSN>(stack, ovf, sp, stride, left_first ? right : left);
            ++sp;
            return left_first ? left : right;
        }
        if (hl) return left;
        if (hr) return right;
        if (sp == sp_floor) return done;
        --sp; return stack_get<S16, LDSN>(stack, ovf, sp, stride);
    }
    const uint4 *np = SOA ? (const uint4 *) nodes + cur : (const uint4 *) (nodes + cur);
    const uint4 a = np[0], b = np[SOA ? kResNodes : 1], c = np[SOA ? 2 * kResNodes : 2], d = np[SOA ? 3 * kResNodes : 3];
    const float lmin[3] = { u2f(a.x), u2f(a.y), u2f(a.z) }, lmax[3] = { u2f(b.x), u2f(b.y), u2f(b.z) };
    const float rmin[3] = { u2f(c.x), u2f(c.y), u2f(c.z) }, rmax[3] = { u2f(d.x), u2f(d.y), u2f(d.z) };
    const uint32_t left = a.w, right = b.w;
    float tl, tr;
    const bool hl = box_hit(lmin, lmax, r, tbest, tl);
    const bool hr = (int) box_hit(rmin, rmax, r, tbest, tr) & (int) (right != (S16 ? kNoChild16 : kNoChild));
    if (hl && hr) {   // (S16: the caller hands in the halfword address of this thread's column)
        const bool left_first = tl <= tr;
        stack_put<S16, LDSN>(stack, ovf, sp, stride, left_first ? right : left);
        ++sp;
        return left_first ? left : right;
    }
    if (hl) return left;
    if (hr) return right;
    if (sp == sp_floor) return done;
    --sp; return stack_get<S16, LDSN>(stack, ovf, sp, stride);
}

// Closest hit (ANY=false) or occlusion (ANY=true) of one top-level object.  Candidates are every
// primitive hit with t <= maxt; the winner is the smallest t, ties going to the lowest
// (object, shape, face) -- the rule the oracle uses, independent of traversal order.
// `stack + sp * stride` onwards is free for the BLAS traversal of a mesh.
// MESH: 0 = rectangles only, 1 = every shape, 2 = rectangles and triangle meshes (scenes without analytic shapes: no float64 sphere / cylinder code, fewer registers).
template <bool ANY, int MESH, bool MEMO = false, uint32_t STRIDE = 0, bool NOBLAS = false, uint32_t LDSN = 0, bool H16 = false>   // H16: the BLAS are walked through sv.nodes16; NOBLAS: the resident kernels (no mesh behind a BLAS; their stack columns are 16-bit)
DTOF_D bool intersect_object(const SceneView &sv, uint32_t oi, V3 o, V3 d, float time, float maxt, Hit &best,
                             uint32_t *stack, int sp, uint32_t stride, uint32_t *ovf = nullptr) {
    const DObject &ob = sv.objects[oi];
    uint32_t first = ob.index, count = 1;
    V3 lo = o, ld = d;
    if (ob.kind == OBJ_INSTANCE) {
        float m[12], inv[12];
        if (MEMO && oi == sv.memo_obj) instance_memo_load(sv, inv);
        else {
            DTOF_STAT(8); DTOF_STAT_WAVE(9);
            instance_matrix(ob, time, m);
            affine_inverse(m, inv);
        }
        lo = xf_point(inv, o); ld = xf_vector(inv, d);
        const DGroup &g = sv.groups[ob.index];
        first = g.first_shape; count = g.n_shapes;
    }
    bool found = false;
    for (uint32_t k = 0; k < count; ++k) {
        const DShape &sh = sv.shapes[first + k];
        float t, u, v;
        if (sh.kind == SHAPE_RECT) {
            DTOF_STAT(12); DTOF_STAT_WAVE(13);
            if (rect_hit(sh, lo, ld, maxt, t, u, v)) {
                if (ANY) return true;
                if (t < best.t || (t == best.t && !found && best.obj != 0xffffffffu && oi < best.obj)) {
                    best.t = t; best.u = u; best.v = v; best.obj = oi; best.shape = k; best.prim = 0; found = true;
                }
            }
            continue;
        }
        if (!MESH) continue;   // instantiations for rectangle-only scenes carry no triangle / sphere code at all
        if (MESH == 1 && sh.kind == SHAPE_DISK) {
            if (disk_hit(sh, lo, ld, maxt, t, u, v)) {
                if (ANY) return true;
                if (t < best.t || (t == best.t && !found && best.obj != 0xffffffffu && oi < best.obj)) {
                    best.t = t; best.u = u; best.v = v; best.obj = oi; best.shape = k; best.prim = 0; found = true;
                }
            }
            continue;
        }
        if (MESH == 1 && sh.kind == SHAPE_CYLINDER) {
            if (cylinder_hit(sh, lo, ld, maxt, t)) {
                if (ANY) return true;
                if (t < best.t || (t == best.t && !found && best.obj != 0xffffffffu && oi < best.obj)) {
                    best.t = t; best.u = 0.f; best.v = 0.f; best.obj = oi; best.shape = k; best.prim = 0; found = true;
                }
            }
            continue;
        }
        if (MESH == 1 && sh.kind == SHAPE_SPHERE) {
            if (sphere_hit<ANY>(sh, lo, ld, maxt, t)) {
                if (ANY) return true;
                if (t < best.t || (t == best.t && !found && best.obj != 0xffffffffu && oi < best.obj)) {
                    best.t = t; best.u = 0.f; best.v = 0.f; best.obj = oi; best.shape = k; best.prim = 0; found = true;
                }
            }
            continue;
        }
        // cull with the mesh's own (padded) bounds: TLAS boxes of moving instances are the union over the whole
        // motion and let many rays through that miss the mesh at their time
        const SlabRay lr = slab_ray(lo, ld);
        float t_entry;
        if (!box_hit(sh.bmin, sh.bmax, lr, ANY ? maxt : best.t, t_entry)) continue;
        // `face` of the best hit so far IF it lies on this very mesh (ties between two of its triangles go to the lower face)
        uint32_t best_face = 0xffffffffu;
        DTOF_STAT(5); DTOF_STAT_WAVE(10);
        auto test = [&](uint32_t f) -> bool {
            DTOF_STAT(6); DTOF_STAT_WAVE(11);
            if (!tri_hit(sv.isect[sh.first_tri + f], lo, ld, maxt, t, u, v)) return false;
            if (ANY) return true;
            const uint32_t face = sv.tris[sh.first_tri + f].face;   // the triangle's index in the mesh's own order (the BLAS permutes them): decides ties
            bool take = t < best.t;
            if (t == best.t) take = best_face != 0xffffffffu ? face < best_face : (!found && best.obj != 0xffffffffu && oi < best.obj);
            if (take) { best.t = t; best.u = u; best.v = v; best.obj = oi; best.shape = k; best.prim = f; best_face = face; found = true; }
            return false;
        };
        if (sh.blas_root == kNoChild) {
            for (uint32_t f = 0; f < sh.n_tris; ++f) if (test(f)) return true;
            continue;
        }
        if (NOBLAS) continue;
        // BLAS: same node format and while-while shape as the TLAS loop below
        constexpr uint32_t kDone = 0x7fffffffu;
        uint32_t cur = sh.blas_root; int bsp = sp;
        for (;;) {
            while (!(cur & kLeafFlag) && cur != kDone) {
                DTOF_STAT(7); DTOF_STAT_WAVE(15);
                cur = node_step<false, STRIDE, false, LDSN, H16>(H16 ? (const BvhNode *) sv.nodes16 : sv.nodes, cur, lr, ANY ? maxt : best.t, stack, bsp, sp, stride, kDone, ovf);
            }
            if (cur == kDone) break;
            uint32_t f0 = (cur & ~kLeafFlag) >> kBlasLeafBits, fn = (cur & ((1u << kBlasLeafBits) - 1u)) + 1u;
            for (uint32_t f = f0; f < f0 + fn; ++f) if (test(f)) return true;
            if (bsp == sp) break;
            --bsp; cur = stack_get<false, LDSN>(stack, ovf, bsp, stride);
        }
    }
    return found;
}

// TLAS traversal; `stack` is a per-thread LDS column (stride blockDim.x).
template <bool ANY, int MESH, bool MEMO = false, bool SOA = false, uint32_t STRIDE = 0, bool S16 = false, uint32_t LDSN = 0, bool TL = false, bool H16 = false, bool DEFER = false>   // DEFER: objects whose TLAS leaf carries kLeafBlas are not entered -- their indices go to `cand` (up to four; a fifth is entered on the spot) for trace_deferred in a second, dense launch; H16: nodes read from sv.nodes16 (the TLAS too, unless TL); TL: `tlas` = a copy of the TLAS nodes in LDS (the BLAS stay where sv.nodes points); SOA: the TLAS nodes are the LDS planes of the resident stage (binary nodes only); STRIDE: the block size, if the kernel knows it; S16: 16-bit references / stack; LDSN: see stack_put
DTOF_D bool trace_scene(const SceneView &sv, uint32_t *stack, V3 o, V3 d, float time, float maxt, Hit &best, uint32_t *ovf = nullptr, const BvhNode *tlas = nullptr, uint4 *cand = nullptr) {
    best.t = maxt; best.u = best.v = 0.f; best.obj = 0xffffffffu; best.shape = 0; best.prim = 0;
    if (sv.n_nodes == 0) return false;
    const SlabRay r = slab_ray(o, d);
    // "while-while" traversal: every lane first descends inner nodes until it holds a leaf (or is done), THEN the
    // lanes that hold a leaf run the expensive object intersection together -- the wave does not pay the leaf
    // body once per node step of its slowest lane.
    constexpr uint32_t kDone = S16 ? kDone16 : 0x7fffffffu, kLeaf = S16 ? kLeafFlag16 : kLeafFlag;   // S16: 16-bit child references and stack entries (encode_child16)
    int sp = 0;
    uint32_t cur = 0;
    const uint32_t stride = STRIDE ? STRIDE : blockDim.x;
    DTOF_STAT(0);
    for (;;) {
        while (!(cur & kLeaf) && cur != kDone) {
            DTOF_STAT(1); DTOF_STAT_WAVE(2);
            cur = TL ? node_step<SOA, STRIDE, S16, LDSN>(tlas, cur, r, best.t, stack, sp, 0, stride, kDone, ovf)
                     : node_step<SOA, STRIDE, S16, LDSN, H16>(H16 ? (const BvhNode *) sv.nodes16 : sv.nodes, cur, r, best.t, stack, sp, 0, stride, kDone, ovf);
        }
        if (cur == kDone) break;
        DTOF_STAT(3); DTOF_STAT_WAVE(4);
        bool put_aside = false;
        if (DEFER && (cur & kLeafBlas)) {   // a mesh behind a BLAS: later, with the other rays that reached one
            const uint32_t oi = cur & kLeafObjMask;
            put_aside = true;
            if (cand->x == 0xffffffffu) cand->x = oi; else if (cand->y == 0xffffffffu) cand->y = oi; else if (cand->z == 0xffffffffu) cand->z = oi; else if (cand->w == 0xffffffffu) cand->w = oi;
            else put_aside = false;
        }
        // The kernels with 16-bit stack columns are the resident ones, whose scenes have no mesh behind a BLAS (render_rows throws otherwise): a BLAS walk would push
        // 32-bit references onto those columns, so their instantiations carry none.
        constexpr bool NOBLAS = S16;
        if (!put_aside && intersect_object<ANY, MESH, MEMO, STRIDE, NOBLAS, LDSN, H16>(sv, cur & ~kLeaf & (S16 ? 0xffffu : kLeafObjMask), o, d, time, maxt, best, stack, sp, stride, ovf) && ANY) return true;
        if (sp == 0) break;
        --sp; cur = stack_get<S16, LDSN>(stack, ovf, sp, stride);
    }
    return best.obj != 0xffffffffu;
}


// (A cooperative form of the small-mesh triangle loops -- one wave-uniform traversal whose 12-triangle loops are shared out over idle lanes -- was built and
// measured slower in round 3; it is parked as tools/experiments/r03_coop_triangles.patch with its numbers in profiles/r03_coop_triangles_ab.txt.)

// Scene query of a kernel whose call site is wave-uniform; `active` says whether this lane has a ray.
template <bool ANY, int MESH, bool MEMO = false, bool SOA = false, uint32_t STRIDE = 0, uint32_t LDSN = 0, bool TL = false, bool H16 = false, bool DEFER = false>
DTOF_D bool trace_rays(const SceneView &sv, uint32_t *stack, bool active, V3 o, V3 d, float time, float maxt, Hit &best, uint32_t *ovf = nullptr, const BvhNode *tlas = nullptr, uint4 *cand = nullptr) {
    bool r = false;
    if (active) r = trace_scene<ANY, MESH, MEMO, SOA, STRIDE, false, LDSN, TL, H16, DEFER>(sv, stack, o, d, time, maxt, best, ovf, tlas, cand);
    return r;
}
// The second launch of a DEFER pair: the objects a ray's TLAS walk put aside, entered one after the other with the hit the first launch found (closest hit: `best` as it
// stands, its distance culls; occlusion: any hit ends the ray).  Every lane of the launch has at least one such object: the BLAS walks run with full waves.
template <bool ANY, int MESH, uint32_t STRIDE, uint32_t LDSN, bool H16>
DTOF_D bool trace_deferred(const SceneView &sv, uint32_t *stack, uint4 cand, V3 o, V3 d, float time, float maxt, Hit &best, uint32_t *ovf) {
    const uint32_t stride = STRIDE ? STRIDE : blockDim.x;
    const uint32_t c[4] = { cand.x, cand.y, cand.z, cand.w };
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        if (c[i] == 0xffffffffu) break;
        if (intersect_object<ANY, MESH, false, STRIDE, false, LDSN, H16>(sv, c[i], o, d, time, maxt, best, stack, 0, stride, ovf) && ANY) return true;
    }
    return best.obj != 0xffffffffu;
}


// Rectangle-only scenes of a handful of top-level objects (the five walls of the Cornell room of C2): no TLAS walk.  Every lane tests
// every object in index order -- a loop whose trip count and addresses are wave-uniform (the records' source: below).  No stack, no divergence: for <= 8 rectangles the
// ~40 instructions per rectangle cost less than the ~55 per node step + ~60 per leaf visit of the binary tree at 0.5 lane utilisation.
// Hits are those of trace_scene bit for bit: same rect_hit arithmetic, smallest t wins, ties go to the lowest object index
// (ascending order + strict <).  Instances take intersect_object (one uniform branch).
// Each rectangle test starts with the z row of its matrix (local z of the ray's origin and direction) and the certain-miss test of dtof_flat_cull.h; when no active lane
// of the wave can hit the rectangle, the wave branches over the rest of the test (the xy rows, the IEEE division, the u / v checks).  Shadow rays of a closed room never
// cross a wall between two points inside it, and rays skip the walls behind them: of the ~37 instructions of a test, ~10 remain.
typedef const uint8_t __attribute__((address_space(4))) *ConstBytes;
// (The rectangle transform as packed multiply-adds -- v_pk_fma_f32 with SGPR-pair operands -- was built behind a switch, bit-exact, and measured on C2: 3 % fewer VALU
// instructions, but spill loads / stores per wave 157 -> 580 and the frame 1.53 -> 1.65 ms, profiles/r03_flat_packed_ab.txt.  Removed.)
typedef float F2 __attribute__((ext_vector_type(2)));
struct FlatRecord { F2 c0, c1, c2, c3; };   // (x, y) entries of the four columns of a rectangle's matrix as pairs; the z row comes from the DFlatZ table
// the z rows of the point and the direction (xf_point / xf_vector, z components): zrow.x = local z of the origin, zrow.y = that of the direction
DTOF_D F2 flat_zrow(float z0, float z1, float z2, float z3, V3 ro, V3 rd) {
    return F2{ fmaf(z2, ro.z, fmaf(z1, ro.y, fmaf(z0, ro.x, z3))), fmaf(z2, rd.z, fmaf(z1, rd.y, z0 * rd.x)) };
}
// The records come from the scene copy staged in LDS, every lane reading the same address (a broadcast): the matrix entries are then VGPR operands of the
// multiply-adds, which issue at full rate -- as SGPR operands (scalar loads from the blob in global memory, the first form of this loop, removed) each of the 21 costs two
// issue slots (profiles/r03_ubench_valu_rate.txt).
// First the object's z row (ONE ds_read_b128 from the DFlatZ table behind the records) and the certain-miss test; the rest of the record (four ds_read_b128) only
// where a lane of the wave still needs the full test.
// FACTS (k_shade's plan facts, dtof_kernels.h) selects one of two forms:
//   kFactOneWall  the one instance is the memo object of one rectangle.  The table is visited as three segments in ascending index order -- the rectangles below the
//                 wall, the wall, the rectangles above it: the plain rectangles read the world ray where it lies and the wall reads its own ray, so no iteration
//                 selects between the two by copying six registers (profiles/flat_peel_ab.txt).  No DFlatKinds loads, no instance loop.
//   otherwise     one loop that picks each object's ray; the instance marks are two scalar loads (DFlatKinds), the instances are intersected after the rectangles.
// One visit is the same in both, operation for operation.  (Sharing its text as one lambda changes the generic kernels' code; the twelve lines are written twice.)
//   PAIR_RAYS     (closest hit, with a shape of 5 and the wall at 2) the caller vouches that lanes 2k and 2k + 1 are both active or both not and hold the same o, d and
//                 maxt (their times may differ: only the wall reads the time).  The plain rectangles are then split between the two lanes -- the even lane tests 0 and
//                 1, the odd lane 3 and 4, through z-row and record addresses that differ by a per-lane constant -- and the wall is tested by both.  dtof_pair_walk.h
//                 has the argument.  One visit is still the one above, operation for operation.  An occlusion query has no such form and takes the sweep as it is: the
//                 form was built for it and for the queries of iteration 0 and cost more than it saved there, DESIGN 8.3 (k), profiles/pair_walk_ab.txt.
//   ZROW          (a shape of 5 with the wall at 2, not PAIR_RAYS) the caller hands in zq = zrow_mfma of (o, d), computed on the matrix cores in front of a call site
//                 that may be lane-divergent (dtof_zrow_mfma.h).  The plain rectangles' visits take their z row from it -- the same bits -- and read no
//                 DFlatZ row; the wall's visit and the occlusion sweep's out-of-line tail keep flat_zrow.
template <bool ANY, bool MEMO, uint32_t FACTS = 0, bool PAIR_RAYS = false, bool ZROW = false, typename ZQ = NoZrow>
DTOF_D bool trace_flat(const SceneView &sv, ConstBytes flat_table, uint32_t flat_off, uint32_t n_objects, uint32_t *stack, V3 o, V3 d, float time, float maxt, Hit &best, ZQ zq = ZQ{}) {
    best.t = maxt; best.u = best.v = 0.f; best.obj = 0xffffffffu; best.shape = 0; best.prim = 0;
    bool occluded = false;
    DTOF_STAT(0);
    // rect_hit on a rectangle's record, the ray (ro, rd) in its space and z = flat_zrow of it
    auto test = [&](const FlatRecord &rec, uint32_t oi, V3 ro, V3 rd, F2 z) {
        // xf_point / xf_vector, x and y rows: one multiply-add per instruction, in the order of the scalar form
        const F2 lo_xy = F2{ fmaf(rec.c2.x, ro.z, fmaf(rec.c1.x, ro.y, fmaf(rec.c0.x, ro.x, rec.c3.x))), fmaf(rec.c2.y, ro.z, fmaf(rec.c1.y, ro.y, fmaf(rec.c0.y, ro.x, rec.c3.y))) };
        const F2 ld_xy = F2{ fmaf(rec.c2.x, rd.z, fmaf(rec.c1.x, rd.y, rec.c0.x * rd.x)), fmaf(rec.c2.y, rd.z, fmaf(rec.c1.y, rd.y, rec.c0.y * rd.x)) };
        const float t = -z.x / z.y;
        const float u = fmaf(ld_xy.x, t, lo_xy.x), v = fmaf(ld_xy.y, t, lo_xy.y);
        // no short-circuit: four compares and three mask ANDs instead of three exec-mask branches per rectangle (the scalar unit is as busy as the vector units here)
        const bool hit = (int) (t >= 0.f) & (int) (t <= maxt) & (int) (fabsf(u) <= 1.f) & (int) (fabsf(v) <= 1.f);
        if (ANY) occluded |= hit;
        else {
            const bool take = (int) hit & (int) (t < best.t);
            best.t = take ? t : best.t; best.u = take ? u : best.u; best.v = take ? v : best.v; best.obj = take ? oi : best.obj;   // best.shape stays 0: the instances, which may set it, come after the rectangles
        }
    };
    constexpr bool F_ONE_WALL = (FACTS & kFactOneWall) != 0;
    static_assert(!F_ONE_WALL || MEMO, "the one wall is the memo object");
    const DFlatObject *lt = (const DFlatObject *) (sv.base + flat_off);
    const uint4 *zt = (const uint4 *) (lt + n_objects) + 1;   // DFlatZ[n_objects], behind the DFlatKinds record
    constexpr int kStat = ANY ? 16 : 20; (void) kStat;   // (stats builds)
    const float far = flat_cull_far(maxt);
    // (Bounding a closest-hit query's certain-miss test by the nearest hit it holds instead of maxt was built behind a switch and failed the bar in its own
    //  A/B, DESIGN 8.3 (g), profiles/flat_peel_ab.txt.  Removed.)
    uint32_t oi = 0;
    if constexpr (F_ONE_WALL) {
        auto visit = [&](uint32_t k, const V3 &ro, const V3 &rd) {
            const uint4 zr = zt[k];
            const F2 z = flat_zrow(u2f(zr.x), u2f(zr.y), u2f(zr.z), u2f(zr.w), ro, rd);
            const bool need = !flat_certain_miss(z.x, z.y, far);
            DTOF_STAT(kStat); DTOF_STAT_WAVE(kStat + 2);
            if (!need) DTOF_STAT(kStat + 1);
            if (!__ballot(need)) return;   // (uniform) no active lane can hit this rectangle
            DTOF_STAT_WAVE(kStat + 3);
            const uint4 *rp4 = (const uint4 *) (lt + k);
            const uint4 r0 = rp4[0], r1 = rp4[1], r2 = rp4[2], r3 = rp4[3];
            FlatRecord a;
            a.c0 = F2{ u2f(r0.x), u2f(r0.y) }; a.c1 = F2{ u2f(r1.x), u2f(r1.y) }; a.c2 = F2{ u2f(r2.x), u2f(r2.y) }; a.c3 = F2{ u2f(r3.x), u2f(r3.y) };
            test(a, k, ro, rd, z);
        };
        // The table's SHAPE as constants (kFactFlatShape: N objects, the wall at index WALL; DESIGN 8.3 (i), profiles/flat_shape_ab.txt): the walk is straight-line code --
        // no counter, no compare, no pass loop, the z rows and records at immediate offsets.  One visit is still the one above, operation for operation.
        constexpr uint32_t N = flat_shape_count(FACTS), WALL = flat_shape_wall(FACTS);
        constexpr bool PAIR = PAIR_RAYS && kPairWalkCompiled;
        static_assert(!PAIR_RAYS || pair_walk_shape(FACTS), "the pair form is written for five rectangles with the wall at index 2: {0, 1} below it, {3, 4} above");
        static_assert(std::is_same<ZQ, typename std::conditional<ZROW, ZrowQuad, NoZrow>::type>::value, "the z rows come with ZROW and only with it");
        static_assert(!ZROW || (zrow_mfma_shape(FACTS) && !PAIR_RAYS && (ANY ? DTOF_FLAT_SHAPE_ANY : DTOF_FLAT_SHAPE_CLOSEST)), "the MFMA z rows are those of rectangles 0, 1, 3, 4 around the wall at index 2, for the shaped walks");
        if constexpr (N != 0 && ANY && DTOF_FLAT_SHAPE_ANY) {
            // Occlusion query: ONE sweep over the z rows and their certain-miss tests, then ONE branch -- where no lane of the wave needs a full test (every shadow
            // ray of a closed room) the query ends there, unoccluded.  `occluded` is an OR: the tail may run the full tests in any order, and runs them in ascending one.
            const DFlatObject *lts = (const DFlatObject *) (sv.base + flat_off);
            const uint4 *zts = (const uint4 *) (lts + N) + 1;
            float inv[12]; instance_memo_load(sv, inv);
            const V3 wo = xf_point(inv, o), wd = xf_vector(inv, d);
            bool any_need = false;
#pragma unroll
            for (uint32_t k = 0; k < N; ++k) {
                F2 z;
                if constexpr (ZROW) {
                    if (k == WALL) { const uint4 zr = zts[k]; z = flat_zrow(u2f(zr.x), u2f(zr.y), u2f(zr.z), u2f(zr.w), wo, wd); }
                    else z = F2{ zq.o[zrow_slot(k)], zq.d[zrow_slot(k)] };
                } else {
                    const uint4 zr = zts[k];
                    z = k == WALL ? flat_zrow(u2f(zr.x), u2f(zr.y), u2f(zr.z), u2f(zr.w), wo, wd) : flat_zrow(u2f(zr.x), u2f(zr.y), u2f(zr.z), u2f(zr.w), o, d);
                }
                const bool need = !flat_certain_miss(z.x, z.y, far);
                DTOF_STAT(kStat); DTOF_STAT_WAVE(kStat + 2);
                if (!need) DTOF_STAT(kStat + 1);
                any_need |= need;
                if ((k & 1u) != 0) __builtin_amdgcn_sched_barrier(0);   // at most two z rows in flight (four registers each)
            }
            if (!__ballot(any_need)) return false;   // (uniform)
            // the tail, out of line: the rectangles some lane still needs, each with the ray it belongs to (the z row again: the same operations give the same bits)
#pragma unroll 1
            for (uint32_t k = 0; k < N; ++k) {
                const bool is_wall = k == WALL;
                const V3 ro = is_wall ? wo : o, rd = is_wall ? wd : d;
                const uint4 zr = zts[k];
                const F2 z = flat_zrow(u2f(zr.x), u2f(zr.y), u2f(zr.z), u2f(zr.w), ro, rd);
                const bool need = !flat_certain_miss(z.x, z.y, far);
                if (!__ballot(need)) continue;   // (uniform)
                DTOF_STAT_WAVE(kStat + 3);
                const uint4 *rp4 = (const uint4 *) (lts + k);
                const uint4 r0 = rp4[0], r1 = rp4[1], r2 = rp4[2], r3 = rp4[3];
                FlatRecord a;
                a.c0 = F2{ u2f(r0.x), u2f(r0.y) }; a.c1 = F2{ u2f(r1.x), u2f(r1.y) }; a.c2 = F2{ u2f(r2.x), u2f(r2.y) }; a.c3 = F2{ u2f(r3.x), u2f(r3.y) };
                test(a, k, ro, rd, z);
            }
            return occluded;
        } else if constexpr (N != 0 && !ANY && DTOF_FLAT_SHAPE_CLOSEST) {
            // Closest hit: the N visits written out in ascending order (strict < keeps the tie rule), each with its forward skip over the full test
            const DFlatObject *lts = (const DFlatObject *) (sv.base + flat_off);
            const uint4 *zts = (const uint4 *) (lts + N) + 1;
            auto visit_at = [&](uint32_t k, const V3 &ro, const V3 &rd) {
                F2 z;
                if constexpr (ZROW) {
                    if (k != WALL) z = F2{ zq.o[zrow_slot(k)], zq.d[zrow_slot(k)] };
                    else { const uint4 zr = zts[k]; z = flat_zrow(u2f(zr.x), u2f(zr.y), u2f(zr.z), u2f(zr.w), ro, rd); }
                } else {
                    const uint4 zr = zts[k];
                    z = flat_zrow(u2f(zr.x), u2f(zr.y), u2f(zr.z), u2f(zr.w), ro, rd);
                }
                const bool need = !flat_certain_miss(z.x, z.y, far);
                DTOF_STAT(kStat); DTOF_STAT_WAVE(kStat + 2);
                if (!need) DTOF_STAT(kStat + 1);
                if (!__ballot(need)) return;   // (uniform)
                DTOF_STAT_WAVE(kStat + 3);
                const uint4 *rp4 = (const uint4 *) (lts + k);
                const uint4 r0 = rp4[0], r1 = rp4[1], r2 = rp4[2], r3 = rp4[3];
                FlatRecord a;
                a.c0 = F2{ u2f(r0.x), u2f(r0.y) }; a.c1 = F2{ u2f(r1.x), u2f(r1.y) }; a.c2 = F2{ u2f(r2.x), u2f(r2.y) }; a.c3 = F2{ u2f(r3.x), u2f(r3.y) };
                test(a, k, ro, rd, z);
            };
            if constexpr (PAIR) {
                // lower | wall | upper (dtof_pair_walk.h).  The two half walks run as ONE instruction stream: slot s of a lane is rectangle s + 3 * (lane & 1), its z row
                // 48 bytes and its record 192 bytes behind the even lane's, at the same immediate offsets.  The skip over a full test stays a wave-wide ballot.
                const uint32_t first = (__lane_id() & 1u) * (WALL + 1u);
                const DFlatObject *ltp = lts + first;
                const uint4 *ztp = zts + first;
#pragma unroll
                for (uint32_t s = 0; s < 2u; ++s) {
                    const uint4 zr = ztp[s];
                    const F2 z = flat_zrow(u2f(zr.x), u2f(zr.y), u2f(zr.z), u2f(zr.w), o, d);
                    const bool need = !flat_certain_miss(z.x, z.y, far);
                    if (__ballot(need)) {   // (uniform)
                        const uint4 *rp4 = (const uint4 *) (ltp + s);
                        const uint4 r0 = rp4[0], r1 = rp4[1], r2 = rp4[2], r3 = rp4[3];
                        FlatRecord a;
                        a.c0 = F2{ u2f(r0.x), u2f(r0.y) }; a.c1 = F2{ u2f(r1.x), u2f(r1.y) }; a.c2 = F2{ u2f(r2.x), u2f(r2.y) }; a.c3 = F2{ u2f(r3.x), u2f(r3.y) };
                        test(a, first + s, o, d, z);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                // every lane takes the even lane's state (quad_perm [0, 0, 2, 2]) and keeps the odd lane's (quad_perm [1, 1, 3, 3]) for the merge: two broadcasts, no
                // select on the parity -- an exchange (quad_perm [1, 0, 3, 2]) would need eight of those to order the two halves
                FlatBest upper;
                upper.t = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(best.t), 0xf5, 0xf, 0xf, false));
                upper.u = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(best.u), 0xf5, 0xf, 0xf, false));
                upper.v = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(best.v), 0xf5, 0xf, 0xf, false));
                upper.obj = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) best.obj, 0xf5, 0xf, 0xf, false);
                best.t = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(best.t), 0xa0, 0xf, 0xf, false));
                best.u = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(best.u), 0xa0, 0xf, 0xf, false));
                best.v = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(best.v), 0xa0, 0xf, 0xf, false));
                best.obj = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) best.obj, 0xa0, 0xf, 0xf, false);
                {
                    float inv[12]; instance_memo_load(sv, inv);
                    const V3 wo = xf_point(inv, o), wd = xf_vector(inv, d);
                    visit_at(WALL, wo, wd);
                }
                __builtin_amdgcn_sched_barrier(0);
                FlatBest b{ best.t, best.u, best.v, best.obj };
                pair_merge_upper(b, upper);
                best.t = b.t; best.u = b.u; best.v = b.v; best.obj = b.obj;
                return best.obj != 0xffffffffu;
            }
#pragma unroll
            for (uint32_t k = 0; k < N; ++k) {
                if (k == WALL) {
                    float inv[12]; instance_memo_load(sv, inv);
                    const V3 wo = xf_point(inv, o), wd = xf_vector(inv, d);
                    visit_at(k, wo, wd);
                } else visit_at(k, o, d);
                __builtin_amdgcn_sched_barrier(0);   // one visit's reads at a time: hoisted together they take the kernel past its register cap
            }
            return best.obj != 0xffffffffu;
        }
        const uint32_t wall = sv.memo_obj;   // < n_objects: a bit of the table's memo mask (kFactOneWall)
        // ONE copy of the plain rectangles' body, run for both segments (two passes of an outer loop the compiler must keep: written out or unrolled, the three bodies
        // of each of the three call sites take C2's kernel to its register cap and two values to scratch); the wall's body, with its ray, sits behind the first pass.
#pragma unroll 1
        for (uint32_t seg = 0; seg < 2u; ++seg) {
            const uint32_t end = seg ? n_objects : wall;
            for (; oi < end; ++oi) visit(oi, o, d);
            if (seg == 0) {
                float inv[12]; instance_memo_load(sv, inv);
                const V3 wo = xf_point(inv, o), wd = xf_vector(inv, d);
                visit(oi++, wo, wd);
            }
        }
    } else {
        // Instances are noted in a mask and intersected after the rectangles: the tie rule of intersect_object (equal t goes to the lower object index) does not depend on
        // the order of the visits.  The one memoised instance of one rectangle is visited in the loop, its ray moved there first as intersect_object does (instance.cpp:101-114).
        typedef const DFlatObject __attribute__((address_space(4))) *ConstFlat;
        const DFlatKinds __attribute__((address_space(4))) *kinds = (const DFlatKinds __attribute__((address_space(4))) *) ((ConstFlat) flat_table + n_objects);
        const uint32_t memo_bit = MEMO && sv.memo_obj < 32u ? 1u << sv.memo_obj : 0u, memo_objs = kinds->memo & memo_bit;
        uint32_t instances = kinds->general | (kinds->memo & ~memo_bit);
        for (; oi < n_objects; ++oi) {
            if ((instances >> oi) & 1u) continue;   // (uniform)
            V3 ro = o, rd = d;
            if ((memo_objs >> oi) & 1u) {
                float inv[12]; instance_memo_load(sv, inv);
                ro = xf_point(inv, o); rd = xf_vector(inv, d);
            }
            const uint4 zr = zt[oi];
            const F2 z = flat_zrow(u2f(zr.x), u2f(zr.y), u2f(zr.z), u2f(zr.w), ro, rd);
            const bool need = !flat_certain_miss(z.x, z.y, far);
            DTOF_STAT(kStat); DTOF_STAT_WAVE(kStat + 2);
            if (!need) DTOF_STAT(kStat + 1);
            if (!__ballot(need)) continue;   // (uniform) no active lane can hit this rectangle
            DTOF_STAT_WAVE(kStat + 3);
            const uint4 *rp4 = (const uint4 *) (lt + oi);
            const uint4 r0 = rp4[0], r1 = rp4[1], r2 = rp4[2], r3 = rp4[3];
            FlatRecord a;
            a.c0 = F2{ u2f(r0.x), u2f(r0.y) }; a.c1 = F2{ u2f(r1.x), u2f(r1.y) }; a.c2 = F2{ u2f(r2.x), u2f(r2.y) }; a.c3 = F2{ u2f(r3.x), u2f(r3.y) };
            test(a, oi, ro, rd, z);
        }
        // (`stack` may be null here -- a kernel compiled with kFactFlat has none: intersect_object<ANY, MESH = false> tests rectangles only and never touches it)
        while (instances) {   // uniform
            const uint32_t k = (uint32_t) __builtin_ctz(instances); instances &= instances - 1u;
            const bool hit = intersect_object<ANY, false, MEMO>(sv, k, o, d, time, maxt, best, stack, 0, blockDim.x);
            if (ANY) occluded |= hit;
        }
    }
    return ANY ? occluded : best.obj != 0xffffffffu;
}

}  // namespace dtof
