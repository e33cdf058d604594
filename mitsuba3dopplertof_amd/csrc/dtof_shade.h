// dtof_shade.h -- the shade kernel of the wavefront path tracer (one bounce of DopplerToFPathIntegrator::sample, src/integrators/dopplertofpath.cpp:130-277,
// and, as the fused first-bounce kernel, lane generation + primary ray + up to four bounces with the path state in registers) and the launch templates
// the dtof_shade_*.hip files instantiate.
#pragma once
#include "dtof_device.h"
#include "dtof_pair_setup.h"
#include <atomic>
#include <initializer_list>
#include <type_traits>

namespace dtof {


// Exclusive prefix of a predicate over the wave = the block (kShadeBlock is one wave; a resident wave owns its segment): ballot + popcount, no LDS, no barrier.
// Returns this lane's slot relative to `running` and advances `running` by the wave's total.
DTOF_D uint32_t wave_append(bool pred, uint32_t &running) {
    const uint64_t mask = __ballot(pred);
    const uint32_t slot = running + (uint32_t) __popcll(mask & ((1ull << __lane_id()) - 1ull));
    running += (uint32_t) __popcll(mask);
    return slot;
}

// BSDF::eval_pdf_sample of the shape's BSDF (src/render/bsdf.cpp:20-29) with every adapter around it -- what one vertex of the bounce loop asks of the material:
// value and density for the emitter direction `wo` (local frame; only when active_em) and the sampled continuation.  SPEC = 0: the diffuse-only scenes' kernels
// (diffuse under an optional twosided); 1: every BSDF / texture / adapter; 2: ... and blendbsdf / twosided with two BSDFs (the chain in a loop over two records).
// One function for k_shade and for the known-answer entry dtof_bsdf_eval (the reference's BSDF unit tests run against it on the GPU).
// The two halves can be asked for separately: active_em = value and density for `wo`, want_sample = the sampled continuation.  Without want_sample (uniform; the
// terminal iteration of k_shade, whose paths nobody continues) the three samples are not read and weight / wo / bs_* come back as zero / false.
// diffuse_wo (HAVE_WO; k_shade under kFactPairSamples only): cosine_hemisphere(s2x, s2y) of this vertex, evaluated ahead of the loop; the diffuse lobe takes it where it would
// call the warp, and everything that depends on the lane (the side test, the density, the weight, the two-sided flip) stays where it is.
struct BsdfOut { V3 val, weight, wo; float pdf, bs_pdf, bs_eta; bool bs_delta, bs_null; };   // bs_null: has_flag(bs.sampled_type, BSDFFlags::Null)
template <int SPEC, bool HAVE_WO = false>
DTOF_D void bsdf_eval_pdf_sample(const SceneView &sv, const DShape *sh, Surface &si, V3 wo, bool active_em, float sample_1, float s2x, float s2y, BsdfOut &out, bool want_sample = true, const V3 *diffuse_wo = nullptr) {
    // ---- the shape's BSDF.  Outermost a `mask`, if any: MaskBSDF (src/bsdfs/mask.cpp:125-163) -- with probability 1 - opacity the path goes straight on (a null
    // interaction: wo = -wi, weight 1, pdf 1 - opacity), otherwise the nested BSDF is sampled with sample1 / opacity; eval and pdf of the nested BSDF are scaled by it.
    const bool masked = SPEC && (sh->flags & SF_MASK);
    bool null_pick = false; float opacity = 1.f;
    if (masked) { opacity = mask_opacity_at(sv, sh, si.u, si.v); null_pick = !(sample_1 < opacity); sample_1 = sample_1 / opacity; }
    // Then a `blendbsdf`, if any (src/bsdfs/blendbsdf.cpp:114-213): eval and pdf are the weighted sums of both nested BSDFs; sample1 <= weight samples bsdf_1 with
    // sample1 / weight, otherwise bsdf_0 with (sample1 - weight) / (1 - weight), and the nested sample goes back as it is.  The chain below runs once per nested BSDF
    // (record 0 = the shape's own, record 1 = the material-only record DShape::blend_other points at).
    // (its own instantiations, SPEC == 2: with the chain inside a loop of run-time trip count the compiler's code for the K = 4 fused kernels gave wrong films
    // on scenes WITHOUT any blend -- found by the random scene sweep; where SPEC != 2 the loop below has one iteration at compile time)
    const bool blend = SPEC == 2 && (sh->flags & SF_BLEND);
    float blend_w = 0.f; bool pick_1 = false;
    if (blend) {
        blend_w = sh->tex_blend ? texture_eval_1(sv, sh->tex_blend << 4, si.u, si.v) : sh->blend_weight;
        blend_w = fmin_(fmax_(blend_w, 0.f), 1.f);   // eval_weight (:213-215)
        pick_1 = sample_1 <= blend_w;
    }
    // `twosided` with two nested BSDFs (twosided.cpp:75-86,111-148): the back side (wi.z < 0) has a record of its own; the flip itself is the chain's
    const DShape *side_sh = (SPEC == 2 && (sh->flags & SF_TWOSIDED2) && si.wi.z < 0.f) ? &sv.shapes[sh->blend_other] : sh;
    const V3 wi_plain = si.wi, wo_plain = wo;
    V3 bsdf_val = mk(0, 0, 0), bsdf_weight = mk(0, 0, 0), bs_wo = mk(0, 0, 0);
    float bsdf_pdf = 0.f, bs_pdf = 0.f, bs_eta = 0.f; bool bs_delta = false, bs_null = false;   // bs_null: has_flag(bs.sampled_type, BSDFFlags::Null)
    V3 val_0 = mk(0, 0, 0), keep_weight = mk(0, 0, 0), keep_wo = mk(0, 0, 0); float pdf_0 = 0.f, keep_pdf = 0.f, keep_eta = 0.f; bool keep_delta = false, keep_null = false;
    for (int pass = 0; pass < (SPEC == 2 && blend ? 2 : 1); ++pass) {
        const DShape *bsh = pass ? &sv.shapes[sh->blend_other] : side_sh;
        const float s1 = !blend ? sample_1 : (pass ? sample_1 / blend_w : (sample_1 - blend_w) / (1.f - blend_w));
        si.wi = wi_plain; wo = wo_plain;
        // ---- BSDF eval_pdf + sample (twosided.cpp:111-148,219-258; diffuse.cpp:101-125,160-180)
        bool twosided = bsh->flags & SF_TWOSIDED;
        // NormalMap (src/bsdfs/normalmap.cpp:110-179) around the plain BSDF, itself inside the two-sided adapter if there is one: the adapter's flip of
        // wi.z / wo.z comes first (twosided.cpp:111-148), then wi and wo move into the frame of the normal map; the sampled direction comes back the
        // same way.  A direction that changes sides between the two frames is a light leak: no value, no density, no weight.
        const bool nmap = SPEC && (bsh->flags & (SF_NORMALMAP | SF_BUMPMAP));   // BumpMap (src/bsdfs/bumpmap.cpp:114-197) wraps its nested BSDF the same way
        LocalFrame nf; V3 wo_flipped = wo; bool nm_back = false;
        if (nmap) {
            nf = (bsh->flags & SF_BUMPMAP) ? bumpmap_frame(sv, bsh, si) : normalmap_frame(sv, bsh, si);
            nm_back = twosided && si.wi.z < 0.f;
            V3 wi_f = si.wi;
            if (nm_back) { wi_f.z = -wi_f.z; wo_flipped.z = -wo_flipped.z; }
            si.wi = frame_to_local(nf, wi_f);
            wo = frame_to_local(nf, wo_flipped);
            twosided = false;
        }
        float wiz = si.wi.z, woz = wo.z;
        if (twosided) { woz = mulsign(woz, wiz); wiz = fabsf(wiz); }
        V3 refl = mk(bsh->refl[0], bsh->refl[1], bsh->refl[2]);
        if (SPEC && (bsh->nonlinear >> 1)) refl = texture_eval(sv, (bsh->nonlinear >> 1) << 4, si.u, si.v);   // m_reflectance->eval(si)
        HitMaterial hm;   // specular colours and roughness of this hit: constants, or the textures on those slots (SPEC instantiations only)
        if (SPEC) hm = material_at(sv, bsh, si.u, si.v);
        bsdf_val = mk(0, 0, 0); bsdf_weight = mk(0, 0, 0); bs_wo = mk(0, 0, 0);
        bsdf_pdf = 0.f; bs_pdf = 0.f; bs_eta = 0.f; bs_delta = false; bs_null = false;
        if (SPEC && bsh->bsdf == BSDF_CONDUCTOR) {
            // SmoothConductor::sample (conductor.cpp:226-277) under TwoSidedBRDF::sample; eval / pdf of a delta lobe are zero
            const float cos_theta_i = twosided ? fabsf(si.wi.z) : si.wi.z;
            if (want_sample && cos_theta_i > 0.f) {
                bs_wo = mk(-si.wi.x, -si.wi.y, si.wi.z);   // reflect(wi); the two-sided flips of wi.z and wo.z cancel
                bs_eta = 1.f; bs_pdf = 1.f; bs_delta = true;
                bsdf_weight = mk(hm.spec_refl[0] * fresnel_conductor(cos_theta_i, bsh->cond_eta[0], bsh->cond_k[0]),
                                 hm.spec_refl[1] * fresnel_conductor(cos_theta_i, bsh->cond_eta[1], bsh->cond_k[1]),
                                 hm.spec_refl[2] * fresnel_conductor(cos_theta_i, bsh->cond_eta[2], bsh->cond_k[2]));
            }
        } else if (SPEC && bsh->bsdf == BSDF_DIELECTRIC) {
            // SmoothDielectric::sample (dielectric.cpp:231-338), TransportMode::Radiance
            if (want_sample) {
            float r_i, cos_theta_t, eta_it, eta_ti;
            fresnel_dielectric(si.wi.z, bsh->diel_eta, r_i, cos_theta_t, eta_it, eta_ti);
            const float t_i = 1.f - r_i;
            const bool selected_r = s1 <= r_i;
            bs_pdf = selected_r ? r_i : t_i; bs_delta = true;
            bs_wo = selected_r ? mk(-si.wi.x, -si.wi.y, si.wi.z) : mk(-eta_ti * si.wi.x, -eta_ti * si.wi.y, cos_theta_t);
            bs_eta = selected_r ? 1.f : eta_it;
            const float f2 = sqr(eta_ti);
            bsdf_weight = selected_r ? mk(hm.spec_refl[0], hm.spec_refl[1], hm.spec_refl[2])
                                     : mk(hm.spec_trans[0] * f2, hm.spec_trans[1] * f2, hm.spec_trans[2] * f2);
            }
        } else if (SPEC && bsh->bsdf == BSDF_NULL) {
            // Null::sample (null.cpp:42-66): straight on, weight 1, pdf 1, a null (and with it a delta) lobe; eval and pdf are zero (:68-79)
            if (want_sample) { bs_wo = mk(-si.wi.x, -si.wi.y, -si.wi.z); bs_eta = 1.f; bs_pdf = 1.f; bs_delta = true; bs_null = true; bsdf_weight = mk(1.f, 1.f, 1.f); }
        } else if (SPEC && bsh->bsdf == BSDF_THINDIELECTRIC) {
            // ThinDielectric::sample (thindielectric.cpp:173-226): the reflectance of the slab with all internal bounces, wo = -wi
            if (want_sample) {
            float r, t1, t2, t3;
            fresnel_dielectric(fabsf(si.wi.z), bsh->diel_eta, r, t1, t2, t3);
            r *= 2.f / (1.f + r);
            const bool selected_r = s1 <= r;
            bs_pdf = selected_r ? r : 1.f - r; bs_delta = true; bs_eta = 1.f;
            bs_null = !selected_r;   // bs.sampled_type = select(selected_r, DeltaReflection, Null) (:179)
            bs_wo = selected_r ? mk(-si.wi.x, -si.wi.y, si.wi.z) : mk(-si.wi.x, -si.wi.y, -si.wi.z);
            bsdf_weight = selected_r ? mk(hm.spec_refl[0], hm.spec_refl[1], hm.spec_refl[2]) : mk(hm.spec_trans[0], hm.spec_trans[1], hm.spec_trans[2]);
            }
        } else if (SPEC && bsh->bsdf == BSDF_ROUGHDIELECTRIC) {
            // RoughDielectric::eval_pdf / sample (roughdielectric.cpp:240-346,503-611): glossy reflection and transmission lobes
            const Ggx g = mf_make((bsh->flags & SF_BECKMANN) ? MF_BECKMANN : MF_GGX, hm.alpha_u, hm.alpha_v, !(bsh->flags & SF_SAMPLE_ALL));
            const V3 wi = si.wi;
            if (active_em) rough_dielectric_eval_pdf(g, bsh, hm, wi, wo, bsdf_val, bsdf_pdf);
            if (want_sample && wi.z != 0.f) {
                float mpdf;
                Ggx gs = g;   // sample_distr (:266-269)
                if (!g.visible) { const float sc = 1.2f - .2f * sqrtf(fabsf(wi.z)); gs.au *= sc; gs.av *= sc; }
                const V3 m = ggx_sample(gs, mk(mulsign(wi.x, wi.z), mulsign(wi.y, wi.z), mulsign(wi.z, wi.z)), s2x, s2y, mpdf);
                const float dwm = dot(wi, m);
                float F, cos_theta_t, eta_it, eta_ti; fresnel_dielectric(dwm, bsh->diel_eta, F, cos_theta_t, eta_it, eta_ti);
                const bool selected_r = s1 <= F;
                bs_pdf = mpdf * (selected_r ? F : 1.f - F);
                bs_eta = selected_r ? 1.f : eta_it;
                float dwh_dwo; V3 w;
                if (selected_r) {
                    bs_wo = mk(fmaf(m.x, 2.f * dwm, -wi.x), fmaf(m.y, 2.f * dwm, -wi.y), fmaf(m.z, 2.f * dwm, -wi.z));   // reflect(wi, m)
                    w = mk(hm.spec_refl[0], hm.spec_refl[1], hm.spec_refl[2]);
                    dwh_dwo = rcp(4.f * dot(bs_wo, m));
                } else {
                    const float k = fmaf(dwm, eta_ti, cos_theta_t);                                                         // refract(wi, m, cos_theta_t, eta_ti)
                    bs_wo = mk(fmaf(m.x, k, -(wi.x * eta_ti)), fmaf(m.y, k, -(wi.y * eta_ti)), fmaf(m.z, k, -(wi.z * eta_ti)));
                    const float f2 = sqr(eta_ti);
                    w = mk(f2 * hm.spec_trans[0], f2 * hm.spec_trans[1], f2 * hm.spec_trans[2]);
                    const float dom = dot(bs_wo, m);
                    dwh_dwo = (sqr(bs_eta) * dom) / sqr(dwm + bs_eta * dom);
                }
                // :345-349: smith_g1(wo, m) with visible normals, else G(wi, wo, m) dot(wi, m) / (cos_theta_i cos_theta(m))
                const float g1 = g.visible ? ggx_smith_g1(g, bs_wo, m) : ggx_smith_g1(g, wi, m) * ggx_smith_g1(g, bs_wo, m) * dwm / (wi.z * m.z);
                bs_pdf *= fabsf(dwh_dwo);
                if (mpdf != 0.f) bsdf_weight = w * g1;
            }
        } else if (SPEC && bsh->bsdf == BSDF_ROUGHCONDUCTOR) {
            // RoughConductor::eval / pdf / sample (roughconductor.cpp:229-415), GGX + visible normals, under TwoSidedBRDF
            V3 wi = si.wi, wo_l = wo;
            if (twosided && wi.z < 0.f) { wi.z = -wi.z; wo_l.z = -wo_l.z; }
            const Ggx g = mf_make((bsh->flags & SF_BECKMANN) ? MF_BECKMANN : MF_GGX, hm.alpha_u, hm.alpha_v, !(bsh->flags & SF_SAMPLE_ALL));
            if (wi.z > 0.f && wo_l.z > 0.f) {
                const V3 H = normalize(wo_l + wi);
                const float D = ggx_eval(g, H);
                if (D != 0.f) {
                    const float G = ggx_smith_g1(g, wi, H) * ggx_smith_g1(g, wo_l, H);
                    const float result = D * G / (4.f * wi.z), c = dot(wi, H);
                    bsdf_val = mk(fresnel_conductor(c, bsh->cond_eta[0], bsh->cond_k[0]) * (result * hm.spec_refl[0]),
                                  fresnel_conductor(c, bsh->cond_eta[1], bsh->cond_k[1]) * (result * hm.spec_refl[1]),
                                  fresnel_conductor(c, bsh->cond_eta[2], bsh->cond_k[2]) * (result * hm.spec_refl[2]));
                }
                if (dot(wi, H) > 0.f && dot(wo_l, H) > 0.f) bsdf_pdf = g.visible ? ggx_eval(g, H) * ggx_smith_g1(g, wi, H) / (4.f * wi.z) : ggx_pdf(g, wi, H) / (4.f * dot(wo_l, H));   // :405-409
            }
            if (want_sample && wi.z > 0.f) {
                float mpdf;
                const V3 m = ggx_sample(g, wi, s2x, s2y, mpdf);
                const float dwm = dot(wi, m);
                const V3 r = mk(fmaf(m.x, 2.f * dwm, -wi.x), fmaf(m.y, 2.f * dwm, -wi.y), fmaf(m.z, 2.f * dwm, -wi.z));   // reflect(wi, m)
                bs_wo = r; bs_eta = 1.f;
                const bool ok = mpdf != 0.f && r.z > 0.f;
                const float weight = g.visible ? ggx_smith_g1(g, r, m) : ggx_smith_g1(g, wi, m) * ggx_smith_g1(g, r, m) * dwm / (wi.z * m.z);   // :260-265
                bs_pdf = mpdf / (4.f * dot(r, m));
                if (ok) bsdf_weight = mk(fresnel_conductor(dwm, bsh->cond_eta[0], bsh->cond_k[0]) * (weight * hm.spec_refl[0]),
                                         fresnel_conductor(dwm, bsh->cond_eta[1], bsh->cond_k[1]) * (weight * hm.spec_refl[1]),
                                         fresnel_conductor(dwm, bsh->cond_eta[2], bsh->cond_k[2]) * (weight * hm.spec_refl[2]));
                if (twosided && si.wi.z < 0.f) bs_wo.z = -bs_wo.z;
            }
        } else if (SPEC && bsh->bsdf == BSDF_ROUGHPLASTIC) {
            // RoughPlastic::eval / pdf / sample (roughplastic.cpp:259-421), GGX + visible normals, under TwoSidedBRDF
            V3 wi = si.wi, wo_l = wo;
            if (twosided && wi.z < 0.f) { wi.z = -wi.z; wo_l.z = -wo_l.z; }
            const Ggx g = mf_make((bsh->flags & SF_BECKMANN) ? MF_BECKMANN : MF_GGX, hm.alpha_u, hm.alpha_u, !(bsh->flags & SF_SAMPLE_ALL));
            const float *table = (const float *) (sv.base + bsh->rough_table);
            const float w = bsh->spec_sampling_weight, ir = bsh->fdr_int;
            const V3 diff = (bsh->nonlinear & 1u) ? mk(refl.x / (1.f - refl.x * ir), refl.y / (1.f - refl.y * ir), refl.z / (1.f - refl.z * ir))
                                          : mk(refl.x / (1.f - ir), refl.y / (1.f - ir), refl.z / (1.f - ir));
            if (wi.z > 0.f) {
                const float t_i = lerp_gather64(table, wi.z);
                float prob_specular = (1.f - t_i) * w, prob_diffuse = t_i * (1.f - w);
                prob_specular = prob_specular / (prob_specular + prob_diffuse);
                prob_diffuse = 1.f - prob_specular;
                if (wo_l.z > 0.f) rough_plastic_eval_pdf(g, bsh, hm, table, diff, wi, wo_l, t_i, prob_specular, prob_diffuse, bsdf_val, bsdf_pdf);
                if (want_sample) {
                if (s1 < prob_specular) {
                    float mpdf; const V3 m = ggx_sample(g, wi, s2x, s2y, mpdf);
                    const float dwm = dot(wi, m);
                    bs_wo = mk(fmaf(m.x, 2.f * dwm, -wi.x), fmaf(m.y, 2.f * dwm, -wi.y), fmaf(m.z, 2.f * dwm, -wi.z));   // reflect(wi, m)
                } else bs_wo = cosine_hemisphere(s2x, s2y);
                bs_eta = 1.f;
                V3 value = mk(0, 0, 0);
                if (bs_wo.z > 0.f) rough_plastic_eval_pdf(g, bsh, hm, table, diff, wi, bs_wo, t_i, prob_specular, prob_diffuse, value, bs_pdf);
                if (bs_pdf > 0.f) bsdf_weight = value * rcp(bs_pdf);                  // Spectrum / Float = multiplication by the reciprocal
                if (twosided && si.wi.z < 0.f) bs_wo.z = -bs_wo.z;
                }
            }
        } else if (SPEC && bsh->bsdf == BSDF_PLASTIC) {
            // SmoothPlastic::eval / pdf / sample (plastic.cpp:219-360) under TwoSidedBRDF; wiz / woz are already flipped
            float f_i, t1, t2, t3;
            fresnel_dielectric(wiz, bsh->diel_eta, f_i, t1, t2, t3);
            const float w = bsh->spec_sampling_weight, fdr = bsh->fdr_int;
            const V3 diff = (bsh->nonlinear & 1u) ? mk(refl.x / (1.f - refl.x * fdr), refl.y / (1.f - refl.y * fdr), refl.z / (1.f - refl.z * fdr))
                                          : mk(refl.x / (1.f - fdr), refl.y / (1.f - fdr), refl.z / (1.f - fdr));
            if (wiz > 0.f && woz > 0.f) {
                float f_o; fresnel_dielectric(woz, bsh->diel_eta, f_o, t1, t2, t3);
                const float k = kInvPi * woz * bsh->inv_eta_2 * (1.f - f_i) * (1.f - f_o);
                bsdf_val = mk(diff.x * k, diff.y * k, diff.z * k);
                const float prob_specular = f_i * w; float prob_diffuse = (1.f - f_i) * (1.f - w);
                prob_diffuse = prob_diffuse / (prob_specular + prob_diffuse);
                bsdf_pdf = kInvPi * woz * prob_diffuse;
            }
            if (want_sample && wiz > 0.f) {
                float prob_specular = f_i * w, prob_diffuse = (1.f - f_i) * (1.f - w);
                prob_specular = prob_specular / (prob_specular + prob_diffuse);
                prob_diffuse = 1.f - prob_specular;
                bs_eta = 1.f;
                if (s1 < prob_specular) {
                    bs_wo = mk(-si.wi.x, -si.wi.y, wiz);
                    bs_pdf = prob_specular; bs_delta = true;
                    const float value = f_i / bs_pdf;
                    bsdf_weight = mk(value * hm.spec_refl[0], value * hm.spec_refl[1], value * hm.spec_refl[2]);
                } else {
                    bs_wo = cosine_hemisphere(s2x, s2y);
                    bs_pdf = prob_diffuse * (kInvPi * bs_wo.z);
                    float f_o; fresnel_dielectric(bs_wo.z, bsh->diel_eta, f_o, t1, t2, t3);
                    const float k = bsh->inv_eta_2 * (1.f - f_i) * (1.f - f_o) / prob_diffuse;
                    bsdf_weight = mk(diff.x * k, diff.y * k, diff.z * k);
                }
                if (twosided) bs_wo.z = mulsign(bs_wo.z, si.wi.z);
            }
        } else {
            if (wiz > 0.f && woz > 0.f) { bsdf_val = mk(refl.x * kInvPi * woz, refl.y * kInvPi * woz, refl.z * kInvPi * woz); bsdf_pdf = kInvPi * woz; }
            if (want_sample && wiz > 0.f) {
                if constexpr (HAVE_WO) bs_wo = *diffuse_wo; else
                bs_wo = cosine_hemisphere(s2x, s2y);
                bs_pdf = kInvPi * bs_wo.z;
                bs_eta = 1.f;
                if (bs_pdf > 0.f) bsdf_weight = refl;
                if (twosided) bs_wo.z = mulsign(bs_wo.z, si.wi.z);
            }
        }
        if (nmap) {
            if (!(wo_flipped.z * wo.z > 0.f)) { bsdf_val = mk(0, 0, 0); bsdf_pdf = 0.f; }
            if (bsdf_weight.x != 0.f || bsdf_weight.y != 0.f || bsdf_weight.z != 0.f) {   // active &= any(weight != 0): a zero sample goes back as it is
                const V3 pw = frame_to_world(nf, bs_wo);
                if (!(bs_wo.z * pw.z > 0.f)) bsdf_weight = mk(0, 0, 0);
                bs_wo = pw;
            }
            if (nm_back) bs_wo.z = -bs_wo.z;
        }
        if (blend) {
            if ((pass == 1) == pick_1) { keep_weight = bsdf_weight; keep_wo = bs_wo; keep_pdf = bs_pdf; keep_eta = bs_eta; keep_delta = bs_delta; keep_null = bs_null; }
            if (pass == 0) { val_0 = bsdf_val; pdf_0 = bsdf_pdf; }
            else {
                const float w0 = 1.f - blend_w;
                bsdf_val = mk(val_0.x * w0 + bsdf_val.x * blend_w, val_0.y * w0 + bsdf_val.y * blend_w, val_0.z * w0 + bsdf_val.z * blend_w);
                bsdf_pdf = pdf_0 * w0 + bsdf_pdf * blend_w;
                bsdf_weight = keep_weight; bs_wo = keep_wo; bs_pdf = keep_pdf; bs_eta = keep_eta; bs_delta = keep_delta; bs_null = keep_null;
            }
        }
    }
    si.wi = wi_plain;
    if (masked) {
        bsdf_val = bsdf_val * opacity; bsdf_pdf *= opacity;
        if (want_sample && null_pick) { bs_wo = mk(-si.wi.x, -si.wi.y, -si.wi.z); bs_eta = 1.f; bs_pdf = 1.f - opacity; bs_delta = true; bs_null = true; bsdf_weight = mk(1.f, 1.f, 1.f); }
    }
    out.val = bsdf_val; out.pdf = bsdf_pdf; out.weight = bsdf_weight; out.wo = bs_wo; out.bs_pdf = bs_pdf; out.bs_eta = bs_eta; out.bs_delta = bs_delta; out.bs_null = bs_null;
}

// BSDF::eval_pdf_sample over arrays (dtof_bsdf_eval_ex): the function above, as the SPEC instantiation the shade kernels of that level call at every path vertex.
// in, 29 floats per query: wi[3], wo[3] (local frame), sample1, sample2[2], u, v, then the geometry normalmap / bumpmap read: dp_du[3], dp_dv[3], n[3], sh_s[3],
// sh_t[3], sh_n[3]; out, 14 floats: value * cos[3], pdf, sampled wo[3], sample pdf, eta, delta flag, weight[3], null flag.  Each dtof_shade_*.hip file that holds a
// SPEC's shade kernels instantiates its launcher (launch_bsdf_eval_spec<SPEC>), so this compiles next to the code it stands for.
template <int SPEC>
__global__ void k_bsdf_eval(const uint8_t *scene, uint32_t shape_index, const float *in, float *out, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SceneView sv = make_view(scene);
    const float *a = in + (size_t) i * 29;
    Surface si;
    si.p = mk(0, 0, 0); si.wi = mk(a[0], a[1], a[2]); si.u = a[9]; si.v = a[10]; si.shape = &sv.shapes[shape_index];
    si.dp_du = mk(a[11], a[12], a[13]); si.dp_dv = mk(a[14], a[15], a[16]); si.n = mk(a[17], a[18], a[19]);
    si.sh_s = mk(a[20], a[21], a[22]); si.sh_t = mk(a[23], a[24], a[25]); si.sh_n = mk(a[26], a[27], a[28]);
    BsdfOut bo;
    bsdf_eval_pdf_sample<SPEC>(sv, si.shape, si, mk(a[3], a[4], a[5]), true, a[6], a[7], a[8], bo, true);   // both halves
    float *w = out + (size_t) i * 14;
    w[0] = bo.val.x; w[1] = bo.val.y; w[2] = bo.val.z; w[3] = bo.pdf; w[4] = bo.wo.x; w[5] = bo.wo.y; w[6] = bo.wo.z; w[7] = bo.bs_pdf; w[8] = bo.bs_eta;
    w[9] = bo.bs_delta ? 1.f : 0.f; w[10] = bo.weight.x; w[11] = bo.weight.y; w[12] = bo.weight.z; w[13] = bo.bs_null ? 1.f : 0.f;
}
template <int SPEC>
void launch_bsdf_eval_spec(const uint8_t *scene, uint32_t shape_index, const float *in, float *out, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_bsdf_eval<SPEC>, dim3(nblk(n)), dim3(kBlock), 0, s, scene, shape_index, in, out, n);
}

// The emitter side of a path vertex over arrays (dtof_emitter_eval): the functions of dtof_shading.h that k_shade<.., AREA, .., MESH, SPEC, .., FACTS> calls, as that
// instantiation calls them (ONE_EMITTER = its kFactOneEmitter fact).  One thread per query, no LDS.  Each dtof_shade_*.hip file instantiates the launcher for the
// (AREA, MESH, SPEC) combinations of its own shade kernels.
//   mode 0  in 5: ref[3], e1, e2                          out 14: p[3], d[3], dist, pdf (* pmf), delta, weight[3] (* the pick's 1 / probability), usable, picked index
//   mode 1  in 11: prev[3], hit[3], sh_n[3], u, v          out 5: dist, d[3], em_pdf                      (`index` = the hit shape; the previous lobe is not a delta)
//   mode 2  in 3: the direction of the ray that left       out 4: em_pdf, value[3]                        (`index` = the environment emitter; SPEC only)
template <bool AREA, bool MESH, int SPEC, bool ONE_EMITTER>
__global__ void k_emitter_eval(const uint8_t *scene, int mode, uint32_t index, float pmf, const float *in, float *out, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SceneView sv = make_view(scene);
    if (mode == 0) {
        const float *a = in + (size_t) i * 5;
        const EmitterSample es = sample_emitter_direction<AREA, MESH, SPEC, ONE_EMITTER>(sv, mk(a[0], a[1], a[2]), a[3], a[4], pmf);
        float *w = out + (size_t) i * 14;
        w[0] = es.p.x; w[1] = es.p.y; w[2] = es.p.z; w[3] = es.d.x; w[4] = es.d.y; w[5] = es.d.z; w[6] = es.dist; w[7] = es.pdf; w[8] = es.delta ? 1.f : 0.f;
        w[9] = es.weight.x; w[10] = es.weight.y; w[11] = es.weight.z; w[12] = es.usable ? 1.f : 0.f; w[13] = (float) es.index;
    } else if (mode == 1) {
        if constexpr (AREA) {
            const float *a = in + (size_t) i * 11;
            const EmitterHit eh = emitter_pdf_direction<MESH, SPEC>(sv, &sv.shapes[index], mk(a[3], a[4], a[5]), mk(a[6], a[7], a[8]), a[9], a[10], mk(a[0], a[1], a[2]), false, pmf);
            float *w = out + (size_t) i * 5;
            w[0] = eh.dist; w[1] = eh.d.x; w[2] = eh.d.y; w[3] = eh.d.z; w[4] = eh.pdf;
        }
    } else {
        if constexpr (SPEC != 0) {   // the miss term of k_shade
            const float *a = in + (size_t) i * 3;
            const DEmitter &env = sv.emitters[index];
            const bool is_map = env.kind == EMITTER_ENVMAP;
            const V3 rd = mk(a[0], a[1], a[2]);
            const float em_pdf = (is_map ? env_pdf_direction(sv.base, env, rd) : kInvFourPi) * pmf;
            const V3 le = is_map ? env_eval(sv.base, env, rd) : mk(env.intensity[0], env.intensity[1], env.intensity[2]);
            float *w = out + (size_t) i * 4;
            w[0] = em_pdf; w[1] = le.x; w[2] = le.y; w[3] = le.z;
        }
    }
}
template <bool AREA, bool MESH, int SPEC, bool ONE_EMITTER = false>
void launch_emitter_eval_level(const uint8_t *scene, int mode, uint32_t index, float pmf, const float *in, float *out, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL((k_emitter_eval<AREA, MESH, SPEC, ONE_EMITTER>), dim3(nblk(n)), dim3(kBlock), 0, s, scene, mode, index, pmf, in, out, n);
}

// FUSED = false: the "split" pipeline -- shadow rays go to the shadow queue (k_shadow commits them) and the
//                 continuation ray is traced by the next k_trace launch.
// FUSED = true : one kernel per bounce -- the occlusion query and the closest-hit query of the continuation ray
//                 run inline, so neither the shadow queue nor a separate trace launch exists; the state streams
//                 through HBM once per bounce (this is the default: the split kernels are latency-bound on small
//                 scenes and the shadow records alone cost 96 B per path-bounce).
// AREA: the scene has area emitters (emitter-hit term, prev_si state).  KMAX: compile-time bound of the batched modulation variants = films (1 or 4; RenderParams::w_d[k], ::phase[k]);
// both keep the common case -- point lights, one offset -- free of the extra registers.
// MODE 0 = split, 1 = fused, 2 = fused AND first bounce: the lane is generated (sampler seeding, camera ray) and its primary
// ray traced right here, so the 96-byte primary state never makes the round trip through HBM and neither k_generate nor the
// primary k_trace launch exists (`dbg`, if given, receives the camera ray for the lane-dump entry point).
// SPEC: the scene has delta BSDFs (conductor / dielectric): the relative index of refraction along the path and the
// "previous lobe was a delta" flag travel in st_c; instantiated together with AREA and MESH only.
// The arguments of k_shade travel as ONE by-value block and are read through the kernarg segment pointer, re-based once per chunk
// on an offset the compiler cannot see through: the ~170 dwords of parameters (camera matrices, sampler and modulation constants, 17
// queue pointers) are then fetched by scalar loads where they are used, instead of being loaded once ahead of the chunk loop and
// kept alive across it -- which, in the first-bounce instantiation, spilled ~120 SGPRs to VGPR lanes (350 v_writelane / v_readlane).
// RESW != 0: the RESIDENT form of the fused first-bounce kernel for scenes too large to stage whole (Domino: 64 KB of TLAS nodes + 128 KB of
// instance records).  ONE block of RESW waves per CU stays for the whole launch; it copies the TLAS nodes (as four planes, see kResNodes) and
// the block of small records (groups, shapes, emitters, triangles, shading data) into LDS once, then every wave takes 512-lane segments from a
// global counter until none is left -- a wave owns its segment exactly as a one-wave block does, there is no barrier after the stage.  What
// still comes through the vector L1 is the 128-byte instance record of a leaf visit and the queue traffic: the unstaged kernel keeps the CU's
// vector memory path busy 75 - 85 % of the time (TA / TD busy counters, profiles/r03_pmc_domino_fused*.txt) with the four 16-byte node loads
// per step per lane, and waits for it.
// FACTS: the plan facts (dtof_kernels.h: kFact*) this instantiation takes as constants instead of reading them, launch-uniform, from the kernarg segment where they
// are used; the scene facts among them (kFactFlat, kFactOneWall) also reach trace_flat and compute_surface, as a template argument of theirs.  0 = none: every F_* below is then a compile-time `false` in front of the run-time read, and the kernel is the text it was without the parameter.
template <bool LDS, int MODE, bool AREA, int KMAX, bool MESH, int SPEC, int RESW = 0, bool RH16 = false, uint32_t FACTS = 0>   // RH16: the resident stage holds HALF-FLOAT node records (DNode16): a TLAS of up to 2 * kResNodes nodes in the LDS of kResNodes float ones; SPEC: 0 diffuse-only scenes, 1 every BSDF / emitter / texture, 2 = 1 + blendbsdf (the BSDF chain in a loop over two records)
#ifndef DTOF_MESH_WAVES
#define DTOF_MESH_WAVES 3   // waves / SIMD the fused kernels with triangle code are compiled for (A/B: make variant DEFS=-DDTOF_MESH_WAVES=4)
#endif
// History of the every-BSDF kernels (SPEC) with four offset films (KMAX == 4): at three waves per SIMD (168 VGPRs, 240 - 390 spilled registers) their fused instantiations
// produced wrong films on scenes of the random sweep whenever the kernel grew, while the K = 1 kernels, the split pipeline and the same source at two waves stayed exact.
// The cause was not the spill code: the films depended on the INITIAL value of the path-state registers declared without one (`main` / `path` below; right with
// -ftrivial-auto-var-init=zero, NaN with =pattern, profiles/r03_k4_uninitialised.txt).  They are initialised now, and both wave counts are correct (sweeps of 240 .. 1 200
// scenes each).  Two waves stay for these instantiations because they are FASTER there: with four films in registers the 168-VGPR build spills 240 - 390 registers, and
// the K = 4 frames of the every-BSDF scenes take 1 - 10 % longer at three waves (cornell_specular 9.13 -> 9.60 ms, cornell_spot 7.80 -> 8.58; profiles/r03_k4_waves_ab.txt)
// -- the opposite of the K = 1 kernels, which lose 20 - 27 % at two (profiles/r03_spec_waves_ab.txt).
// DTOF_K4_RES_LDS (default 1): the RESIDENT kernels of SEVERAL films (RESW != 0, KMAX > 1) keep neither the K running results nor the K NEE candidates in registers
// (round 4's four-film Domino kernel carried 12 + 12 of them across both traversals of every iteration, in scratch: profiles/r04_pmc_c4_c5.txt).  What is pending across
// the shadow ray is K-INDEPENDENT -- the throughput, the unweighted contribution bsdf_val * em_weight * mis_em and the path length to the emitter
// (dopplertofpath.cpp:214-226: only eval_modulation_weight, :60-77, depends on the film's offset and frequency) = 7 registers -- and the K weights are applied when the
// sample is committed, in the same fmaf order.  The running results live in LDS columns: Domino's stage leaves 44 KiB of the CU's 160 free at 16 waves, kParkWords = 11
// words per thread, which hold 11 of the 12 floats of four RGB results (the twelfth stays a register).  Film state then costs the K = 4 kernel ONE register more than the
// K = 1 kernel's, and a commit is 12 ds_read + 12 ds_write.  0: results and candidates stay in registers, as in every other kernel.
// These kernels decide `want_shadow` from the pending sample (are its three products non-zero?) where every other form compares the candidate with the current result:
// a few more shadow rays, same films -- their shadow-ray counters are NOT comparable with the other forms'.
// (The same pending sample with the running results read-modify-written in q.res, for every several-film first-bounce kernel, was built behind a switch of its own and
// measured no faster than the registers on the four-film Domino frame, 181.9 against 178.9 ms, profiles/r05_k4_film_state.txt.  Removed.)
#ifndef DTOF_K4_RES_LDS
#define DTOF_K4_RES_LDS 1
#endif
__global__ __launch_bounds__(RESW ? RESW * 64 : kShadeBlock, RESW ? RESW / 4 : (MODE == 2 && !MESH && !SPEC && KMAX == 1) ? 4 : (MODE != 0 && MESH) ? ((SPEC && KMAX > 1) ? 2 : DTOF_MESH_WAVES) : 1) void k_shade(ShadeArgs args_by_value) {
    constexpr bool FUSED = MODE != 0, FIRST = MODE == 2;
    static_assert(FACTS == 0 || MODE == 2, "plan facts describe a first-bounce launch");
    constexpr bool F_SINGLE_PASS = (FACTS & kFactSinglePass) != 0, F_DOPPLER_CORR = (FACTS & kFactDopplerCorr) != 0, F_NO_LANE_OUT = (FACTS & kFactNoLaneOutput) != 0;
    constexpr bool F_IDENTITY = (FACTS & kFactIdentityQueue) != 0, F_NO_RR = (FACTS & kFactNoRoulette) != 0, F_CORRELATED = (FACTS & kFactCorrelated) != 0;
    constexpr bool F_WHOLE_PATH = (FACTS & kFactWholePath) != 0, F_ONE_BLOCK = (FACTS & kFactOneBlock) != 0, F_ONE_EMITTER = (FACTS & kFactOneEmitter) != 0;
    constexpr bool F_WAVE_PIXEL = (FACTS & kFactWavePixel) != 0;
    constexpr bool F_FLAT = (FACTS & kFactFlat) != 0, F_ONE_WALL = (FACTS & kFactOneWall) != 0, F_FUSED_SPLAT = (FACTS & kFactFusedSplat) != 0;
    // the routes of the sampler and of the modulation weight are taken inside generate_lane / next_time / modulation_weight, which get FACTS; here:
    constexpr bool F_EMITTER_SAMPLED = (FACTS & kFactEmitterSampled) != 0, F_ID24 = (FACTS & kFactIdShift24) != 0, F_SHIFTS = facts_lane_shifts(FACTS);
    // the two lanes of a pair hold ONE path stream and every draw of the loop comes from it, so the draws -- and the warp of the two that are read --
    // are the pair's, not the lane's.  JUMPS: the draws nobody reads advance the stream by pcg_jump; PAIR: a lane evaluates one iteration's direction, its partner the other's
    constexpr bool F_PAIR = (FACTS & kFactPairSamples) != 0, JUMPS = F_PAIR && DTOF_STREAM_JUMPS, PAIR = F_PAIR && DTOF_PAIR_SAMPLES;
    // ... and (k): the camera ray, which the two lanes of a pair share, splits its plain rectangles between them (trace_flat: PAIR_RAYS)
    constexpr bool WALK_PRIMARY = F_PAIR && DTOF_PAIR_WALK_PRIMARY && pair_walk_shape(FACTS);
    // ... and (l): the pair's piece of lane generation is evaluated once per pair, for the pairs of two chunks at a time (dtof_pair_setup.h).  The block walks its
    // segment from chunk 0 (kFactOneBlock), its lanes are the segment's own (kFactIdentityQueue), and only the diffuse-only kernels generate perspective rays alone
    constexpr bool PAIR_SETUP = F_PAIR && DTOF_PAIR_SETUP && F_ONE_BLOCK && F_IDENTITY && SPEC == 0 && lane_split_facts(FACTS);
    static_assert(kPairChunk == (uint32_t) kShadeBlock, "a chunk of the pair setup is one block of k_shade");
    static_assert(!F_PAIR || F_WAVE_PIXEL, "a lane reads its partner's registers: the whole wave is active where it does");
    static_assert(!F_PAIR || (!AREA && SPEC == 0 && KMAX == 1 && F_ONE_EMITTER), "a diffuse BSDF picks no lobe and a lone point light samples nothing: of an iteration's six draws only s2x and s2y are read");
    static_assert(!F_PAIR || (F_NO_RR && F_CORRELATED && F_DOPPLER_CORR && F_WHOLE_PATH && F_SINGLE_PASS && (FACTS & kFactStratifiedPairs) != 0), "every draw comes from the stream lanes 2k and 2k + 1 share, none is looked at for roulette, no state outlives the launch");
    // ... and (m): the z rows of the plain rectangles for the shadow and continuation rays come from the matrix cores, six MFMAs per query issued in front of the
    // lane-divergent call sites (dtof_zrow_mfma.h; the primary walk keeps the pair form of (k))
    constexpr bool ZROW = FUSED && F_FLAT && zrow_mfma_shape(FACTS & kFactsFlatTable) && DTOF_FLAT_SHAPE_ANY && DTOF_FLAT_SHAPE_CLOSEST;
    constexpr bool F_FRAMES = F_ONE_WALL && DTOF_WALL_FRAMES;   // shading frames precomputed: the wall's once per path, the plain rectangles' on the host (compute_surface)
    static_assert(!F_FLAT || (!MESH && SPEC == 0 && RESW == 0), "trace_flat serves the staged rectangle-only diffuse kernels");
    static_assert(!F_ONE_WALL || F_FLAT, "the one wall is an object of the flat table");
    static_assert(!F_FUSED_SPLAT || KMAX == 1, "the fused splat is the one-film kernels'");
    static_assert(!F_WAVE_PIXEL || F_IDENTITY, "whole waves of one pixel are provable for an identity queue only");
    static_assert(!F_ONE_BLOCK || RESW == 0, "blocks per segment belong to the classic launch");
    constexpr bool RES_LDS = RESW != 0 && KMAX > 1 && DTOF_K4_RES_LDS;   // several films, resident stage: running results in LDS columns, the pending NEE sample K-independent (see above)
    constexpr bool S16 = RESW != 0 && KMAX > 1;                           // ... whose LDS comes from 16-bit traversal stacks (dtof_traverse.h: encode_child16)
    static_assert(!RES_LDS || 3 * KMAX == (int) kParkWords + 1, "the film-state columns hold all but the last float of the K results");
    constexpr bool PARK_ST = DTOF_PARK && RESW == 16 && KMAX == 1;   // the path state no traversal reads waits in LDS columns while the rays are traced: throughput / path length (one film only) ...
    constexpr bool PARK = DTOF_PARK && RESW == 16 && (KMAX == 1 || RES_LDS);   // ... and both PCG streams (several films: behind the film words)
    constexpr uint32_t kRngAt = RES_LDS ? kParkWords : 0u;
    constexpr int KREG = RES_LDS ? 1 : KMAX;                         // film-state registers the lane carries
    constexpr uint32_t kStackStride = RESW ? RESW * 64 : kShadeBlock;   // the block size = the stride of the traversal-stack columns
    static_assert(RESW == 0 || (MODE == 2 && !LDS && MESH), "the resident stage exists for the unstaged fused first-bounce kernel with mesh code");
    static_assert(!RH16 || RESW != 0, "half-float LDS planes belong to the resident stage");
    extern __shared__ uint4 lds[];
    __shared__ uint32_t s_inline_all[(RESW ? RESW : 1) * 2 * kMaxInline];   // FIRST: lanes alive after / shadow rays of every inline iteration but the last (statistics), per wave
    typedef const char __attribute__((address_space(4))) *KernargBytes;
    const KernargBytes kernarg = (KernargBytes) __builtin_amdgcn_kernarg_segment_ptr();
    const ShadeArgs &A0 = *(const ShadeArgs *) kernarg;
    const uint32_t lane_id = RESW ? threadIdx.x & 63u : threadIdx.x, wave_id = RESW ? threadIdx.x >> 6 : 0u;   // one wave per block otherwise
    uint32_t *const s_inline = s_inline_all + wave_id * 2 * kMaxInline;
    const uint32_t stage_words = RESW ? 4u * kResNodes + A0.res_small_words : A0.stage_words;
    // dynamic LDS: [staged scene | resident stage: node planes, record block][fused: instance memo, kMemoWords x 64 words per wave][traversal stack columns][park columns]
    // -- the host sizes every launch with ShadeLds (dtof_kernels.h), the mirror of the offsets derived here (stage_words, memo_words, stack, park)
    // flat scenes with ONE instance (the moving wall of C2): the column holds the instance matrix as well (ShadeLds::classic sizes the LDS accordingly) -- re-deriving it per
    // iteration cost every lane 51 instructions, a hit on the wall now reads it back
    const bool memo_m_lds = F_ONE_WALL || (FUSED && !MESH && !RESW && A0.rp.flat_objects != 0u && A0.rp.memo_obj != 0xffffffffu);
    const uint32_t memo_words = FUSED ? (RESW ? (A0.res_memo ? RESW * kMemoWords * kMemoStride : 0u) : (memo_m_lds ? 2u : 1u) * kMemoWords * kMemoStride) : 0u;
    // per-thread traversal stack column; the resident kernels' columns are 16-bit (halfword address in a uint32_t *: only trace_scene<SOA> / node_step<SOA> touch it)
    // (kFactFlat: no ray query walks a tree -- the launch has no stack columns, launch_shade_plain)
    uint32_t *stack = F_FLAT ? nullptr : S16 ? (uint32_t *) ((uint16_t *) ((uint32_t *) (lds + stage_words) + memo_words) + threadIdx.x) : (uint32_t *) (lds + stage_words) + memo_words + threadIdx.x;
    // One block per 512-lane segment -- or, for a small frame whose whole path runs inline (rp.chunk_blocks = 8: nothing is compacted for a
    // later launch), one block per 64-lane chunk, so that a 1 M-lane frame is 16 384 waves instead of 2 048; the per-segment statistics are
    // then accumulated with atomics into slots the host has zeroed.
    const uint32_t sub = FIRST ? (RESW ? A0.rp.res_units : F_ONE_BLOCK ? 1u : A0.rp.chunk_blocks) : 1u;   // work units per segment: blocks (1 or kSeg / kShadeBlock), resident: what a wave takes from the counter at a time
    const uint32_t unit_lanes = kSeg / sub;
    SceneView sv_res;
    if (RESW) {   // the resident stage: every thread of the block copies, ONE barrier, then the waves go their own ways
        const BlobHeader *gh = (const BlobHeader *) A0.scene;
        if (RH16) {   // two planes of 2 * kResNodes 16-byte pieces: (left box, left child) | (right box, right child)
            const uint4 *gn = (const uint4 *) (A0.scene + gh->off_nodes16);
            const uint32_t n_pieces = gh->n_nodes * 2u;
            for (uint32_t i = threadIdx.x; i < n_pieces; i += blockDim.x) {
                uint4 piece = gn[i];
                if (S16) piece.w = encode_child16(piece.w);
                lds[(i & 1u) * (2u * kResNodes) + (i >> 1)] = piece;
            }
        } else {
        const uint4 *gn = (const uint4 *) (A0.scene + gh->off_nodes);
        const uint32_t n_pieces = gh->n_nodes * 4u;
        for (uint32_t i = threadIdx.x; i < n_pieces; i += blockDim.x) {
            uint4 piece = gn[i];
            if (S16 && (i & 3u) < 2u) piece.w = encode_child16(piece.w);   // left / right child: 16-bit references (dtof_traverse.h), so that the stack columns are 16-bit
            lds[(i & 3u) * kResNodes + (i >> 2)] = piece;
        }
        }
        const uint4 *gs = (const uint4 *) (A0.scene + A0.res_small_off);
        for (uint32_t i = threadIdx.x; i < A0.res_small_words; i += blockDim.x) lds[4u * kResNodes + i] = gs[i];
        __syncthreads();
        const uint8_t *small = (const uint8_t *) (lds + 4u * kResNodes) - A0.res_small_off;   // blob offsets of the copied block resolve into LDS
        sv_res = make_view(A0.scene);
        sv_res.nodes = (const DNode *) lds; sv_res.nodes16 = (const DNode16 *) lds;
        sv_res.groups = (const DGroup *) (small + gh->off_groups); sv_res.shapes = (const DShape *) (small + gh->off_shapes);
        sv_res.tris = (const DTri *) (small + gh->off_tris); sv_res.shading = (const DTriShade *) (small + gh->off_shading);
        sv_res.isect = (const DTriIsect *) (small + gh->off_isect);
        sv_res.emitters = (const DEmitter *) (small + gh->off_emitters);
    }
    for (;;) {   // resident: until the segment counter runs out; otherwise once
    uint32_t seg, sub_index = 0;
    if (RESW) {
        uint32_t taken = 0;
        if (lane_id == 0) taken = atomicAdd(A0.q.seg_counter, 1u);
        uint32_t unit = (uint32_t) __builtin_amdgcn_readfirstlane((int) taken);
        if (unit >= A0.n_seg * sub) break;
        // the units are handed out from the LAST pixel rows to the first: a launch ends with a tail in which the waves run out of work one after the other, and the
        // tail is as long as the last units are expensive -- the top rows of a frame tend to see sky (Domino C4: 34.05 -> 33.77 ms, profiles/r04_domino_waves_batch.txt)
        unit = A0.n_seg * sub - 1u - unit;
        seg = sub > 1 ? unit / sub : unit; sub_index = sub > 1 ? unit - seg * sub : 0u;
    } else {
        seg = sub > 1 ? blockIdx.x / sub : blockIdx.x; sub_index = sub > 1 ? blockIdx.x - seg * sub : 0u;
    }
    const uint32_t count = seg_count(F_IDENTITY ? nullptr : A0.count_in, seg, A0.rp.n_lanes);
    uint32_t n_alive = 0, n_shadow = 0;
    if (FIRST && lane_id < 2 * kMaxInline) s_inline[lane_id] = 0;   // a wave's own slots: no barrier needed
    if (count != 0) {
    const uint8_t *base = LDS ? stage_scene(A0.scene, A0.scene_bytes, lds) : A0.scene;
    SceneView sv = RESW ? sv_res : make_view(base);
    if (FUSED) { sv.memo_obj = A0.rp.memo_obj; sv.memo = (float *) (lds + stage_words) + (RESW ? wave_id * kMemoWords * kMemoStride + lane_id : threadIdx.x); sv.memo_m = memo_m_lds; }
    const bool have_memo = F_ONE_WALL || (FUSED && sv.memo_obj != 0xffffffffu);
    // ZROW: the matrix-side operands of the plain rectangles' z rows, per-lane constants of the launch, read from the staged DFlatZ table with every lane active
    typename std::conditional<ZROW, ZrowOperands, NoZrow>::type zrow_m;
    if constexpr (ZROW) zrow_m = zrow_operands((const uint4 *) ((const DFlatObject *) (sv.base + A0.rp.flat_off) + flat_shape_count(FACTS)) + 1);
    PairPart pair_carried = pair_part_zero();   // PAIR_SETUP: the pair values an even chunk leaves for itself and for the chunk after it
    for (uint32_t cbase = sub > 1 ? sub_index * unit_lanes : 0u; cbase < (sub > 1 ? (sub_index + 1) * unit_lanes < count ? (sub_index + 1) * unit_lanes : count : count); cbase += kShadeBlock) {
    uint32_t rebase = 0;
    asm volatile("" : "+s"(rebase));
    const ShadeArgs &A = *(const ShadeArgs *) (kernarg + rebase);
    const RenderParams &rp = A.rp; const Queues &q = A.q;
    const uint32_t *const qin = F_IDENTITY ? nullptr : A.qin; uint32_t *const qout = A.qout; const uint32_t depth0 = A.depth, trace_next_last = F_WHOLE_PATH ? 0u : A.trace_next;
    LaneDebug *const dbg = F_NO_LANE_OUT ? nullptr : A.dbg;
    const uint32_t flat = FUSED && !MESH ? rp.flat_objects : 0u;   // != 0: the scene's object count, every ray tests them all (trace_flat)
    uint32_t j = cbase + lane_id;
    bool in_range = F_WAVE_PIXEL || j < count;   // (the fact: count - cbase >= 64 in every chunk)
    bool alive = false, want_shadow = false;
    uint32_t l = 0;
    // every register of the path state starts defined: a build of these kernels whose K = 4 every-BSDF instantiations ran at three waves per SIMD produced films that
    // depended on the initial value of `main` / `path` below (wrong with the registers' garbage, NaN with -ftrivial-auto-var-init=pattern, right with =zero;
    // profiles/r03_k4_uninitialised.txt) although no source path reads them before they are assigned
    float4 sha = make_float4(0.f, 0.f, 0.f, 0.f), shb = sha, nra = sha, nrb = sha; float3 cand[KREG];
#pragma unroll
    for (int k = 0; k < KREG; ++k) cand[k] = make_float3(0.f, 0.f, 0.f);
    float3 rbase[KREG];   // FIRST: the result a lane ends this launch with if its NEE candidate is not committed
#pragma unroll
    for (int k = 0; k < KREG; ++k) rbase[k] = make_float3(0.f, 0.f, 0.f);
    // RES_LDS: the pending emitter sample without its modulation weights -- throughput before the bounce, bsdf_val * em_weight * mis_em, path length to the emitter
    V3 pend_thr = mk(0, 0, 0), pend_v = mk(0, 0, 0); float pend_len = 0.f;
    float *const park = RES_LDS || PARK ? (float *) (lds + stage_words) + memo_words + A0.res_park_off + threadIdx.x : nullptr;   // word f of this thread at park[f * kStackStride]
    float res_last = 0.f;   // RES_LDS: the one float of the K results that has no LDS word (film KMAX - 1, blue)
    // the lane's running result of film k: its LDS words (RES_LDS), a register (the other first-bounce kernels), its q.res record (the bounce kernels).  (Plain `if`s: under
    // `if constexpr` the two closures capture other variables in the RES_LDS kernels than elsewhere, and the register allocation of every kernel moves with that.  Where
    // KREG is 1, the [k] of the register form sits behind a return / an else of a constant.)
    auto res_get = [&](int k) -> float4 {
        if (RES_LDS) return make_float4(park[(3 * k) * kStackStride], park[(3 * k + 1) * kStackStride], 3 * k + 2 < (int) kParkWords ? park[(3 * k + 2) * kStackStride] : res_last, 0.f);
        if (!FIRST) return q.res[(size_t) k * q.capacity + l];
        const float3 r = rbase[k]; return make_float4(r.x, r.y, r.z, 0.f);
    };
    auto res_put = [&](int k, float4 v) {
        if (RES_LDS) {
            park[(3 * k) * kStackStride] = v.x; park[(3 * k + 1) * kStackStride] = v.y;
            if (3 * k + 2 < (int) kParkWords) park[(3 * k + 2) * kStackStride] = v.z; else res_last = v.z;
        }
        else if (FIRST) rbase[k] = make_float3(v.x, v.y, v.z);
        else q.res[(size_t) k * q.capacity + l] = v;
    };
    // RES_LDS: the lane's results are zero (a new path; a path of null interactions that ends invalid)
    auto res_clear = [&]() {
#pragma unroll
        for (uint32_t f = 0; f < kParkWords; ++f) park[f * kStackStride] = 0.f;
        res_last = 0.f;
    };
    if constexpr (RES_LDS) res_clear();
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // Path state of the lane.  MODE 2 runs rp.inline_iters iterations of the bounce loop right here ("megakernel" head): between them the
    // state stays in these registers instead of making the round trip through the queues in HBM; after the last one the survivors are
    // written out and compacted exactly as before, for the bounce kernels (MODE 1) to continue with.
    uint32_t hid = 0xffffffffu; float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = make_float4(0.f, 0.f, 1.f, 0.f), st = ra; uint4 hh = make_uint4(0u, 0u, 0u, 0u); Rng main = { 0ull, 1ull }, path = { 0ull, 1ull };
    float4 stb_reg = make_float4(0.f, 0.f, 0.f, 1.f); float2 stc_reg = make_float2(1.f, 1.f);   // prev_si.p | prev_bsdf_pdf, eta | prev_bsdf_delta
    uint32_t *const parku = (uint32_t *) park;
    auto park_store = [&]() {   // PARK: both streams (state + 32-bit selector: inc = sel << 1 | 1) and throughput / path length leave the registers
        parku[kRngAt * kStackStride] = (uint32_t) main.state; parku[(kRngAt + 1) * kStackStride] = (uint32_t) (main.state >> 32); parku[(kRngAt + 2) * kStackStride] = (uint32_t) (main.inc >> 1);
        parku[(kRngAt + 3) * kStackStride] = (uint32_t) path.state; parku[(kRngAt + 4) * kStackStride] = (uint32_t) (path.state >> 32); parku[(kRngAt + 5) * kStackStride] = (uint32_t) (path.inc >> 1);
        if (PARK_ST) { park[6 * kStackStride] = st.x; park[7 * kStackStride] = st.y; park[8 * kStackStride] = st.z; park[9 * kStackStride] = st.w; }
    };
    auto park_load = [&]() {
        main.state = (uint64_t) parku[kRngAt * kStackStride] | ((uint64_t) parku[(kRngAt + 1) * kStackStride] << 32); main.inc = ((uint64_t) parku[(kRngAt + 2) * kStackStride] << 1) | 1u;
        path.state = (uint64_t) parku[(kRngAt + 3) * kStackStride] | ((uint64_t) parku[(kRngAt + 4) * kStackStride] << 32); path.inc = ((uint64_t) parku[(kRngAt + 5) * kStackStride] << 1) | 1u;
        if (PARK_ST) st = make_float4(park[6 * kStackStride], park[7 * kStackStride], park[8 * kStackStride], park[9 * kStackStride]);
    };
    // valid_ray (dopplertofpath.cpp:101-102,252-253,279-282): starts as "the environment is visible", becomes true at the first vertex whose sampled lobe is not
    // BSDFFlags::Null (a `mask` that lets the path through, the transmission of a `thindielectric`); a path that ends without it returns 0 (and alpha 0).  Only the
    // every-BSDF kernels (SPEC) can sample a null lobe: elsewhere a lane is valid as soon as its primary ray hits something.  FIRST: this register; the bounce
    // kernels carry it as bit 1 of st_c.y (bit 0 = prev_bsdf_delta).
    const bool valid_start = SPEC && rp.has_env && !rp.hide_emitters;
    bool valid_reg = valid_start;
    float memo_m[12], memo_inv[12];   // instance memo: the one instance's matrix and inverse at this lane's ray time
    // kFactOneWall: the wall's unit normal and tangent at this lane's ray time, and the plain rectangles' frames (DFlatFrame[n] behind DFlatObject[n], DFlatKinds, DFlatZ[n])
    typename std::conditional<F_FRAMES, WallFrames, NoFrames>::type wf;
    if constexpr (F_FRAMES) wall_frames_init(wf, sv, rp.flat_off, rp.flat_objects);
    V3 pair_wo = mk(0.f, 0.f, 1.f), pair_wo_next = pair_wo;   // PAIR: the BSDF's sampled direction (local frame) of the iteration that runs and of the one after it
    bool lane_on = in_range;
#ifdef DTOF_TRAVERSAL_STATS   // development builds: lanes without a path carry a poison pattern; DTOF_POISON_CHECK counts it wherever path state is written out (statistic [14])
    constexpr uint64_t kPoisonState = 0xdeadbeefcafef00dull;
    if (!in_range) { main.state = path.state = kPoisonState; const float pz = u2f(0x7fc0dead); ra = rb = st = make_float4(pz, pz, pz, pz); }
#define DTOF_POISON_CHECK() do { if (main.state == kPoisonState || path.state == kPoisonState || f2u(st.x) == 0x7fc0deadu || f2u(ra.x) == 0x7fc0deadu) DTOF_STAT(14); } while (0)
#else
#define DTOF_POISON_CHECK() ((void) 0)
#endif
    // the wave's 64 lanes are the 64-aligned lanes [lane_base + seg * 512 + cbase, + 64): samples of one pixel if spp is a multiple of 64
    // ... AND the whole wave is in range: the pair swap of the correlated seeding (generate_lane) reads the partner lane, which a ragged tail
    // (dtof_sample_lanes with an odd count) would leave inactive.  Under a pixel list (rp.pixels) the same test holds: spp is a power of two >= 64 and lane_base a
    // multiple of spp (batches are whole pixels), so the wave's 64 virtual lanes lie in ONE listed pixel and global_lane maps them to 64 consecutive, 64-aligned
    // global lanes of it -- what generate_lane's pair swap and pixel_info<true> need.  (A launch with a list never carries kFactWavePixel: FramePlan::launch_facts.)
    const bool wave_pixel = F_WAVE_PIXEL || (FIRST && rp.spp_log2 != 0xffffffffu && rp.spp_log2 >= 6 && (rp.lane_base & 63u) == 0 && count - cbase >= (uint32_t) kShadeBlock);
    // Fused splat (uniform): this launch runs the whole path of its lanes (nobody continues) and the host handed in the film -- the wave reduces the footprint
    // values of its 64 samples itself and issues the film atomics, the result never goes through q.res / q.pos and the splat kernel's round trip through HBM
    const bool fuse_splat = F_FUSED_SPLAT || (FIRST && A.film != nullptr);
    float2 pos_reg = make_float2(0.f, 0.f);
    if (in_range) {
        l = qin ? qin[seg * kSeg + j] : seg * kSeg + j;
        if (FIRST) {
            // (PAIR_SETUP: l = seg * kSeg + cbase + lane_id, and the global lane is the virtual one under the lane shifts)
            PrimaryLane pl;
            if constexpr (PAIR_SETUP) pl = pair_setup_chunk<FACTS, DTOF_PAIR_SETUP_BPERMUTE != 0>(rp, rp.lane_base + seg * kSeg + cbase, lane_id, ((cbase >> 6) & 1u) != 0, pair_carried);
            else pl = generate_lane<SPEC == 0, FACTS>(rp, global_lane<FACTS>(rp, rp.lane_base + l), wave_pixel, rp.lane_base + l);
            ra = pl.ray_a; rb = pl.ray_b; main = pl.main; path = pl.path; st = make_float4(1.f, 1.f, 1.f, 0.f);
            if constexpr (PAIR) {
                // Iteration i reads the draws at offsets 6 i + 3 and 6 i + 4 of the stream generate_lane leaves (s2x, s2y) and warps them; the terminal iteration reads none.
                // The even lane of a pair does that for iteration 0, the odd lane for iteration 1 -- one instruction stream, the state chosen by parity -- and each hands
                // its three components to both (quad_perm [0, 0, 2, 2] and [1, 1, 3, 3]; kFactWavePixel: every lane of the wave is active here).  The stream is dead afterwards.
                const bool odd = lane_id & 1u;   // (lane_base, the segment and the chunk are even: the lane's parity is its parity in the wave)
                uint64_t sx;
                if constexpr (JUMPS) {   // pcg_jump<9> in the odd lanes, pcg_jump<3> in the even ones: ONE jump whose two constants the parity selects
                    constexpr uint64_t m3 = pcg_pow(3), g3 = pcg_geom(3), m9 = pcg_pow(9), g9 = pcg_geom(9);
                    sx = path.state * (odd ? m9 : m3) + path.inc * (odd ? g9 : g3);
                } else {
                    uint64_t s3 = path.state;
                    for (int i = 0; i < 3; ++i) s3 = s3 * kPcgMult + path.inc;
                    uint64_t s9 = s3;
                    for (int i = 0; i < 6; ++i) s9 = s9 * kPcgMult + path.inc;
                    sx = odd ? s9 : s3;
                }
                const uint64_t sy = sx * kPcgMult + path.inc;
                const V3 mine = cosine_hemisphere(pcg_output_f32(sx), pcg_output_f32(sy));
                pair_wo = mk(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mine.x), 0xa0, 0xf, 0xf, false)),
                             __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mine.y), 0xa0, 0xf, 0xf, false)),
                             __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mine.z), 0xa0, 0xf, 0xf, false)));
                pair_wo_next = mk(__int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mine.x), 0xf5, 0xf, 0xf, false)),
                                  __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mine.y), 0xf5, 0xf, 0xf, false)),
                                  __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mine.z), 0xf5, 0xf, 0xf, false)));
            }
            if (PARK) park_store();
            pos_reg = pl.pos;
            if (!fuse_splat) {   // what the later launches (stream selectors) and the splat kernels (sample position) read
                q.pos[l] = pl.pos;
                q.rng_b[l] = make_uint2((uint32_t) (main.inc >> 1), (uint32_t) (path.inc >> 1));
            }
            if (dbg) {
                LaneDebug &o = dbg[l];
                o.time = ra.w; o.ray_o[0] = ra.x; o.ray_o[1] = ra.y; o.ray_o[2] = ra.z; o.ray_d[0] = rb.x; o.ray_d[1] = rb.y; o.ray_d[2] = rb.z;
            }
            if (have_memo) instance_memo_fill(sv, ra.w, memo_m, memo_inv);
            if constexpr (F_FRAMES) wall_frames_fill(wf, sv, memo_m, memo_inv);   // (dtof_shading.h)
            Hit h;
            // (WALK_PRIMARY: kFactStratifiedPairs gives lanes 2k and 2k + 1 one pixel jitter from the stream they share and times of their own -- the same o, d and maxt --
            //  and kFactWavePixel has every lane of the wave here)
            bool found = (F_FLAT || flat) ? trace_flat<false, true, FACTS & kFactsFlatTable, WALK_PRIMARY>(sv, (ConstBytes) A.scene + rp.flat_off, rp.flat_off, flat, stack, mk(ra.x, ra.y, ra.z), mk(rb.x, rb.y, rb.z), ra.w, rb.w, h)
                              : trace_scene<false, MESH, FUSED, RESW != 0, kStackStride, S16, 0u, false, RH16>(sv, stack, mk(ra.x, ra.y, ra.z), mk(rb.x, rb.y, rb.z), ra.w, rb.w, h);
            hh = make_uint4(f2u(h.t), f2u(h.u), f2u(h.v), h.prim);
            hid = found ? (h.obj | (h.shape << (F_ID24 ? 24u : q.id_shift))) : 0xffffffffu;
        }
    }
    const uint32_t n_inline = FIRST ? rp.inline_iters : 1u;
    for (uint32_t it = 0; ; ++it) {
    const uint32_t depth = depth0 + it;
    const bool last = it + 1 >= n_inline;                 // uniform
    const uint32_t trace_next = last ? trace_next_last : 1u;
    // the TERMINAL iteration (uniform; RenderParams::terminal): nothing continues a path after it and nobody reads what the second half of the bounce leaves behind.
    // Where it still samples an emitter (active_next: the last iteration that runs in a scene without surface emitters) it keeps the emitter-hit term, the emitter
    // sample with its two draws, the BSDF's value and density for it and the NEE candidate with its shadow ray; where it does not, only the emitter-hit term.
    const bool terminal = last && (F_WHOLE_PATH || rp.terminal != 0);
    alive = false; want_shadow = false;
    if (lane_on) {
        if (PARK) park_load();
        if (!FIRST) {
            hid = q.hit_id[l];
            if (hid != 0xffffffffu) {
                ra = q.ray_a[l]; rb = q.ray_b[l]; hh = load_hit<MESH>(q, l); st = q.st_a[l];
                const uint4 rs = q.rng_a[l]; const uint2 ri = q.rng_b[l];
                main.state = (uint64_t) rs.x | ((uint64_t) rs.y << 32); main.inc = ((uint64_t) ri.x << 1) | 1u;
                path.state = (uint64_t) rs.z | ((uint64_t) rs.w << 32); path.inc = ((uint64_t) ri.y << 1) | 1u;
            }
        }
        if (!F_SINGLE_PASS && hid == 0xffffffffu && rp.n_passes > 1) {
            // several passes: the streams are carried into the next pass, so the six draws the reference makes for EVERY lane that is
            // active at the entry of an iteration (App. A step 5; both streams advance on each, correlated.cpp:156-161) also happen
            // for the lanes whose ray misses (single-pass renders drop the state of a finished path instead)
            if (!FIRST) {
                const uint4 rs = q.rng_a[l]; const uint2 ri = q.rng_b[l];
                main.state = (uint64_t) rs.x | ((uint64_t) rs.y << 32); main.inc = ((uint64_t) ri.x << 1) | 1u;
                path.state = (uint64_t) rs.z | ((uint64_t) rs.w << 32); path.inc = ((uint64_t) ri.y << 1) | 1u;
            }
            const bool one = rp.integrator != 0 || rp.sampler_kind != SAMPLER_CORRELATED;
            main.state = pcg_jump6(main.state, main.inc); if (!one) path.state = pcg_jump6(path.state, path.inc);   // six steps at once: the same integers
            q.rng_a[l] = make_uint4((uint32_t) main.state, (uint32_t) (main.state >> 32), (uint32_t) path.state, (uint32_t) (path.state >> 32));
        }
        // valid_ray of the lane as it enters this iteration
        const bool valid_in = FIRST ? valid_reg : (SPEC ? (depth > 0 ? q.st_c[l].y >= 2.f : valid_start) : depth > 0);
        if (hid == 0xffffffffu) {   // the path ends here: nothing validates it any more
            if (SPEC && !valid_in && depth > 0) {   // select(valid_ray, result, 0) (:279-282): what the path gathered behind null interactions does not count
                if constexpr (RES_LDS) res_clear();
                else {
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) res_put(k, zero4);
                }
            }
            if (!F_NO_LANE_OUT && rp.want_valid) q.valid_out[l] = make_float4(valid_in ? 1.f : 0.f, 0.f, 0.f, 0.f);
        }
        if (SPEC && hid == 0xffffffffu && rp.has_env && valid_in) {
            // The ray left the scene: si.emitter(scene) is the environment (dopplertofpath.cpp:150-168).  DirectionSample(scene, si, prev_si)
            // points along the ray; ConstantBackgroundEmitter::pdf_direction is the uniform-sphere density (constant.cpp:150-155).  A path that
            // is not valid here (hidden emitters, and nothing but null interactions so far -- a primary ray above all) returns 0 whatever it adds
            // (valid_ray, :101-102,279-282).
            const float4 stv = FIRST ? st : q.st_a[l];
            const float time_ = FIRST ? ra.w : q.ray_a[l].w;
            float prev_pdf = 1.f; bool pdelta = true;
            if (depth > 0) { prev_pdf = FIRST ? stb_reg.w : q.st_b[l].w; pdelta = FIRST ? stc_reg.y != 0.f : ((uint32_t) q.st_c[l].y & 1u) != 0u; }
            const DEmitter &env = sv.emitters[rp.env_index];
            const bool is_map = env.kind == EMITTER_ENVMAP;   // EnvironmentMapEmitter::pdf_direction / eval (envmap.cpp:408-425,299-310) with ds.d = -si.wi = the ray direction
            const V3 rd = FIRST ? mk(rb.x, rb.y, rb.z) : [&] { const float4 b4 = q.ray_b[l]; return mk(b4.x, b4.y, b4.z); }();
            const float em_pdf = pdelta ? 0.f : (is_map ? env_pdf_direction(sv.base, env, rd) : kInvFourPi) * rp.emitter_pmf;
            const float mis_bsdf = mis_weight(prev_pdf, em_pdf);
            const V3 le = prev_pdf > 0.f ? (is_map ? env_eval(sv.base, env, rd) : mk(env.intensity[0], env.intensity[1], env.intensity[2])) : mk(0, 0, 0);
#pragma unroll
            for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) {
                V3 v = le * mis_bsdf;
                if (rp.integrator == 0) v = v * modulation_weight<FACTS>(rp, rp.w_d[k], rp.phase[k], rp.phi_coef[k], rp.w_g[k], time_, stv.w);
                const float4 r = res_get(k);
                res_put(k, make_float4(fmaf(stv.x, v.x, r.x), fmaf(stv.y, v.y, r.y), fmaf(stv.z, v.z, r.z), 0.f));
            }
        }
        if (hid != 0xffffffffu) {   // a miss ends the path (active_next = false, dopplertofpath.cpp:171)
            V3 o = mk(ra.x, ra.y, ra.z), d = mk(rb.x, rb.y, rb.z); float time = ra.w;
            V3 thr = mk(st.x, st.y, st.z); float path_length = st.w;
            float eta_path = 1.f; bool prev_delta = depth == 0;   // dopplertofpath.cpp:103-108: eta = 1, prev_bsdf_delta = true
            if (SPEC && depth > 0) { const float2 sc = FIRST ? stc_reg : q.st_c[l]; eta_path = sc.x; prev_delta = FIRST ? sc.y != 0.f : ((uint32_t) sc.y & 1u) != 0u; }
            bool correlate = F_CORRELATED || (depth + 1) < rp.path_correlation_depth;
            const bool plain = !F_DOPPLER_CORR && rp.integrator != 0;   // `path`: no modulation weight
            const bool single = !F_DOPPLER_CORR && (plain || rp.sampler_kind != SAMPLER_CORRELATED);   // main stream only (path.cpp:197,213-214,273; sampler.h:141-144)
            float t = u2f(hh.x);
            path_length += t * eta_path;   // dopplertofpath.cpp:141 (eta stays 1 without dielectrics)
            bool active_next = F_EMITTER_SAMPLED || depth + 1 < rp.max_depth;   // (the fact: true in every iteration of the launch)

            Surface si;
            if (!FIRST && have_memo) instance_memo_fill(sv, time, memo_m, memo_inv);
            if (FIRST && it > 0 && have_memo && !sv.memo_m) {   // a ray's time does not change along its path: the inverse filled at generation still sits in the LDS column
                instance_matrix(sv.objects[sv.memo_obj], time, memo_m); instance_memo_load(sv, memo_inv);
            }
            // the diffuse-only kernels' terminal iteration reads the cosines wi.z / wo.z and nothing else of the shading frame
            const bool want_frame = SPEC != 0 || !terminal;
            if constexpr (F_FRAMES) compute_surface<MESH, FACTS & kFactOneWall>(sv, hid & ((1u << (F_ID24 ? 24u : q.id_shift)) - 1u), hid >> (F_ID24 ? 24u : q.id_shift), hh.w, t, u2f(hh.y), u2f(hh.z), o, d, time, si, have_memo, memo_m, memo_inv, want_frame, &wf);
            else compute_surface<MESH, FACTS & kFactOneWall>(sv, hid & ((1u << (F_ID24 ? 24u : q.id_shift)) - 1u), hid >> (F_ID24 ? 24u : q.id_shift), hh.w, t, u2f(hh.y), u2f(hh.z), o, d, time, si, have_memo, memo_m, memo_inv, want_frame);
            const DShape *sh = si.shape;

            const float pmf = rp.emitter_pmf;   // m_emitter_pmf (scene.cpp:96)
            // ---- direct emission (dopplertofpath.cpp:150-168 / path.cpp): the hit shape carries an area emitter
            bool res_dirty = false;
            float4 rcur[KREG];   // (RES_LDS: the emitter-hit term goes straight to the LDS columns)
            if (AREA) {
                if constexpr (!RES_LDS) {
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) rcur[k] = res_get(k);
                }
                if (sh->flags & SF_EMITTER) {
                    float4 pb = depth > 0 ? (FIRST ? stb_reg : q.st_b[l]) : make_float4(0.f, 0.f, 0.f, 1.f);   // prev_si.p, prev_bsdf_pdf
                    // DirectionSample(scene, si, prev_si), records.h:173-180; !prev_bsdf_delta: AreaLight::pdf_direction (area.cpp:161-180)
                    const float em_pdf = emitter_pdf_direction<MESH, SPEC>(sv, sh, si.p, si.sh_n, si.u, si.v, mk(pb.x, pb.y, pb.z), prev_delta, pmf).pdf;
                    float mis_bsdf = mis_weight(pb.w, em_pdf);
                    bool on = si.wi.z > 0.f && pb.w > 0.f;                       // AreaLight::eval (area.cpp:82-89), mask prev_bsdf_pdf > 0
                    V3 le = on ? mk(sh->radiance[0], sh->radiance[1], sh->radiance[2]) : mk(0, 0, 0);
                    if (SPEC && on && sh->tex_radiance) le = texture_eval(sv, sh->tex_radiance << 4, si.u, si.v);   // m_radiance->eval(si)
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) {
                        V3 v = le * mis_bsdf;
                        if (!plain) v = v * modulation_weight<FACTS>(rp, rp.w_d[k], rp.phase[k], rp.phi_coef[k], rp.w_g[k], time, path_length);
                        float4 r;
                        if constexpr (RES_LDS) r = res_get(k); else r = rcur[k];
                        const float4 acc = make_float4(fmaf(thr.x, v.x, r.x), fmaf(thr.y, v.y, r.y), fmaf(thr.z, v.z, r.z), 0.f);
                        if constexpr (RES_LDS) res_put(k, acc); else rcur[k] = acc;
                    }
                    res_dirty = !RES_LDS;
                }
            }

            if (terminal && !active_next) {
                // terminal, and no emitter is sampled at this depth: the iteration existed for the emitter-hit term alone.  valid_ray: terminal launches are those of
                // scenes without a null lobe (plan_frame), where every vertex validates its path
                if constexpr (!RES_LDS) if (res_dirty) {
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) res_put(k, rcur[k]);
                }
                if (!F_NO_LANE_OUT && rp.want_valid) q.valid_out[l] = make_float4(1.f, 0.f, 0.f, 0.f);
            } else {
            // ---- emitter sampling (scene.cpp:235-291; point.cpp:118-147; area.cpp:116-159 + shape.cpp:370-384 + rectangle.cpp:152-166)
            // The six draws of this iteration (App. A step 5) come from ONE stream: the main one (`path`, other samplers, correlate = false) or
            // the path-correlated one; next_1d_correlate advances both on every draw (correlated.cpp:156-161), so the stream that is not read
            // is moved six steps at once at the end (pcg_jump6: the same integers as six single steps).
            const bool use_path = !single && correlate;
            Rng sel = use_path ? path : main;
            float e1 = 0.f, e2 = 0.f;   // (F_PAIR: a lone point light reads neither)
            if constexpr (!JUMPS && !PAIR) { e1 = next_f32(sel); e2 = next_f32(sel); }
            // has_flag(bsdf->flags(), BSDFFlags::Smooth) (:178): diffuse, (rough)plastic and roughconductor have a smooth lobe
            bool active_em = active_next && (F_ONE_EMITTER || sv.n_emitters > 0) && (!SPEC || bsdf_is_smooth(sh->bsdf) || ((sh->flags & (SF_BLEND | SF_TWOSIDED2)) && bsdf_is_smooth(sv.shapes[sh->blend_other].bsdf)));   // a blend (a twosided of two BSDFs) has the flags of both
            V3 em_weight = mk(0, 0, 0), wo = mk(0, 0, 0); float ds_dist = 0.f, ds_pdf = 0.f; bool ds_delta = true;
            if (active_em) {
                const EmitterSample es = sample_emitter_direction<AREA, MESH, SPEC, F_ONE_EMITTER>(sv, si.p, e1, e2, pmf);
                const V3 dsp = es.p, dd = es.d;
                em_weight = es.weight; ds_dist = es.dist; ds_pdf = es.pdf; ds_delta = es.delta; active_em = es.usable;
                // Interaction::spawn_ray_to (interaction.h:141-149)
                V3 so = offset_p(si, dsp - si.p);
                V3 sd = dsp - so;
                float sdist = norm(sd);
                sd = sd * rcp(sdist);
                sha = make_float4(so.x, so.y, so.z, sdist * (1.f - kShadowEps));
                shb = make_float4(sd.x, sd.y, sd.z, time);
                wo = want_frame ? mk(dot(dd, si.sh_s), dot(dd, si.sh_t), dot(dd, si.sh_n)) : mk(0.f, 0.f, dot(dd, si.sh_n));
            }
            float sample_1 = 0.f, s2x = 0.f, s2y = 0.f;   // terminal: the BSDF is not sampled, and the stream states are dropped with the path
            if constexpr (PAIR) { }   // the direction is in pair_wo
            else if constexpr (JUMPS) {   // e1, e2 and sample_1 are three steps nobody looks at; s2x and s2y are the draws of the same two states as before
                if (!terminal) { sel.state = pcg_jump<3>(sel.state, sel.inc); s2x = next_f32(sel); s2y = pcg_output_f32(sel.state); }
            } else
            if (!terminal) { sample_1 = next_f32(sel); s2x = next_f32(sel); s2y = next_f32(sel); }

            // ---- the shape's BSDF with its adapters (mask, blendbsdf, twosided, normalmap / bumpmap): bsdf_eval_pdf_sample above
            BsdfOut bo;
            if constexpr (PAIR) bsdf_eval_pdf_sample<SPEC, true>(sv, sh, si, wo, active_em, sample_1, s2x, s2y, bo, !terminal, &pair_wo);
            else
            bsdf_eval_pdf_sample<SPEC>(sv, sh, si, wo, active_em, sample_1, s2x, s2y, bo, !terminal);
            const V3 bsdf_val = bo.val, bs_wo = bo.wo; V3 bsdf_weight = bo.weight;
            const float bsdf_pdf = bo.pdf, bs_pdf = bo.bs_pdf, bs_eta = bo.bs_eta; const bool bs_delta = bo.bs_delta, bs_null = bo.bs_null;
            // ---- emitter contribution candidate (dopplertofpath.cpp:214-226); committed by k_shadow if unoccluded
            if (active_em) {
                const float mis_em = ds_delta ? 1.f : mis_weight(ds_pdf, bsdf_pdf);   // dopplertofpath.cpp:218-219
                bool nonzero = false;
                if constexpr (RES_LDS) {   // the sample waits for its visibility test WITHOUT the K modulation weights; they are applied at the commit (below), in the order of the loop that follows
                    pend_thr = thr; pend_len = path_length + ds_dist;
                    pend_v = mk(bsdf_val.x * em_weight.x * mis_em, bsdf_val.y * em_weight.y * mis_em, bsdf_val.z * em_weight.z * mis_em);
                    // a sample whose three products are zero adds exactly zero to every film whatever its weights: no visibility test (the register form compares the
                    // candidate with the current result, which also catches a zero weight and a term below the result's last bit -- a few more shadow rays here, same films)
                    nonzero = (int) (pend_thr.x * pend_v.x != 0.f) | (int) (pend_thr.y * pend_v.y != 0.f) | (int) (pend_thr.z * pend_v.z != 0.f);
                } else {
#pragma unroll
                for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) {
                    float4 r = AREA ? rcur[k] : res_get(k);
                    V3 v = mk(bsdf_val.x * em_weight.x * mis_em, bsdf_val.y * em_weight.y * mis_em, bsdf_val.z * em_weight.z * mis_em);
                    if (!plain) { float lw = modulation_weight<FACTS>(rp, rp.w_d[k], rp.phase[k], rp.phi_coef[k], rp.w_g[k], time, path_length + ds_dist); v = v * lw; }
                    float3 c = make_float3(fmaf(thr.x, v.x, r.x), fmaf(thr.y, v.y, r.y), fmaf(thr.z, v.z, r.z));
                    cand[k] = c;
                    nonzero |= f2u(c.x) != f2u(r.x) || f2u(c.y) != f2u(r.y) || f2u(c.z) != f2u(r.z);
                }
                }
                want_shadow = nonzero;   // a candidate identical to the current result needs no visibility test
            }
            if constexpr (!RES_LDS) if (res_dirty) {   // the emitter-hit term stands whether or not the NEE candidate is later committed
#pragma unroll
                for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) res_put(k, rcur[k]);
            }
            if (terminal) {   // the path ends here whatever it sampled; valid_ray as above
                if (!F_NO_LANE_OUT && rp.want_valid) q.valid_out[l] = make_float4(1.f, 0.f, 0.f, 0.f);
            } else {
            // ---- continuation (dopplertofpath.cpp:232-276)
            V3 nd = vfma(si.sh_n, bs_wo.z, vfma(si.sh_t, bs_wo.y, si.sh_s * bs_wo.x));   // Frame::to_world
            V3 no = offset_p(si, nd);
            thr = mk(thr.x * bsdf_weight.x, thr.y * bsdf_weight.y, thr.z * bsdf_weight.z);
            const float eta = eta_path * bs_eta;   // eta *= bs.eta (:252); bs.eta = 0 for the zero-initialised sample when cos_theta_i <= 0
            uint32_t ndepth = depth + 1;
            float thr_max = fmax_(fmax_(thr.x, thr.y), thr.z);
            float rr_prob = fmin_(thr_max * sqr(eta), .95f);
            bool rr_active = !F_NO_RR && ndepth >= rp.rr_depth;   // (the fact: the draw below still advances the stream, its value is not looked at)
            bool rr_continue = true;
            if constexpr (PAIR) { }   // no stream is read again
            else if constexpr (JUMPS) path.state = pcg_jump<2>(sel.state, sel.inc);   // s2y's step and the roulette's: the state the iteration leaves is the one after six steps
            else {
            rr_continue = next_f32(sel) < rr_prob;
            if (use_path) { path.state = sel.state; main.state = pcg_jump6(main.state, main.inc); }
            else { main.state = sel.state; if (!single) path.state = pcg_jump6(path.state, path.inc); }
            }
            if (rr_active) thr = thr * rcp(rr_prob);
            alive = active_next && (!rr_active || rr_continue) && thr_max != 0.f;
            // valid_ray |= active && si.is_valid() && !has_flag(bsdf_sample.sampled_type, BSDFFlags::Null) (:252-253)
            const bool valid_now = !SPEC || valid_in || !bs_null;
            const bool ends = !alive || (last && !trace_next);   // nobody continues this path: what it returns is decided here
            if (SPEC && ends && !valid_now) {   // select(valid_ray, result, 0) (:279-282): neither the emitter-hit term nor this vertex's NEE candidate survives
                want_shadow = false;
                if constexpr (RES_LDS) res_clear();
                else {
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) res_put(k, zero4);
                }
            }
            if (!F_NO_LANE_OUT && ends && rp.want_valid) q.valid_out[l] = make_float4(valid_now ? 1.f : 0.f, 0.f, 0.f, 0.f);
            if (FIRST) valid_reg = valid_now;
            if (alive) {
                nra = make_float4(no.x, no.y, no.z, time); nrb = make_float4(nd.x, nd.y, nd.z, kLargest);
                const float4 sta = make_float4(thr.x, thr.y, thr.z, path_length), stb = make_float4(si.p.x, si.p.y, si.p.z, bs_pdf);
                const float2 stc = make_float2(eta, bs_delta ? 1.f : 0.f);
                if ((!FIRST || last) && trace_next) {   // the state leaves for the queues (an inline iteration keeps it in registers; after the last iteration of the loop nobody reads it)
                    q.ray_a[l] = nra;
                    q.ray_b[l] = nrb;
                    q.st_a[l] = sta;
                    if (AREA) q.st_b[l] = stb;   // prev_si, prev_bsdf_pdf (:256-257)
                    if (SPEC) q.st_c[l] = make_float2(stc.x, stc.y + (valid_now ? 2.f : 0.f));   // eta, prev_bsdf_delta (:252,258) | valid_ray << 1
                }
                if (FIRST) { st = sta; stb_reg = stb; stc_reg = stc; }
                if (PARK) park_store();
                DTOF_POISON_CHECK();   // the state of a path that continues
            }
            if ((alive && (!FIRST || last) && trace_next) || (!F_SINGLE_PASS && rp.n_passes > 1))   // several passes: the state of a finished path is what its lane starts the next pass with
                q.rng_a[l] = make_uint4((uint32_t) main.state, (uint32_t) (main.state >> 32), (uint32_t) path.state, (uint32_t) (path.state >> 32));
            }   // !terminal: continuation
            }   // emitter sampling and what follows it
        }
    }
    if (last) {
        uint32_t slot = wave_append(alive, n_alive);
        if (alive && trace_next) qout[seg * kSeg + slot] = l;
    } else {   // FIRST, one wave per block
        const uint32_t n_on = (uint32_t) __popcll(__ballot(alive));
        if (lane_id == 0) s_inline[2 * it] += n_on;
    }
    if constexpr (FUSED) {
        bool commit = false;
        // (Both rays in ONE traversal loop -- a lane going on with its continuation ray while its neighbours are still in their shadow rays -- was built and measured in
        // round 5 and lost by a third: tools/experiments/r05_pair_traversal.patch, profiles/r05_pair_traversal.txt.)
        // ZROW: every lane of the wave takes part in the MFMAs (uniform control flow; sha / shb are defined in the lanes without a shadow ray, their results unread)
        typename std::conditional<ZROW, ZrowQuad, NoZrow>::type zq_shadow{}, zq_next{};
        if constexpr (ZROW) zq_shadow = zrow_mfma(zrow_m, sha.x, sha.y, sha.z, shb.x, shb.y, shb.z);
        if (want_shadow) {   // test_visibility (scene.cpp:266-271): an unoccluded sample commits its candidate result
            Hit hs;
            commit = (F_FLAT || flat) ? !trace_flat<true, true, FACTS & kFactsFlatTable, false, ZROW, decltype(zq_shadow)>(sv, (ConstBytes) A.scene + rp.flat_off, rp.flat_off, flat, stack, mk(sha.x, sha.y, sha.z), mk(shb.x, shb.y, shb.z), shb.w, sha.w, hs, zq_shadow)
                          : !trace_scene<true, MESH, true, RESW != 0, kStackStride, S16, 0u, false, RH16>(sv, stack, mk(sha.x, sha.y, sha.z), mk(shb.x, shb.y, shb.z), shb.w, sha.w, hs);
        }
        if constexpr (RES_LDS) {   // the committed sample gets its K modulation weights now (dopplertofpath.cpp:221-226) and is added to the films' running results
            if (commit) {
                const bool plain_ = rp.integrator != 0;
#pragma unroll
                for (int k = 0; k < KMAX; ++k) if (k < rp.n_offsets) {
                    V3 v = pend_v;
                    if (!plain_) v = v * modulation_weight<FACTS>(rp, rp.w_d[k], rp.phase[k], rp.phi_coef[k], rp.w_g[k], shb.w, pend_len);   // shb.w: the ray time (the shadow ray carries it)
                    const float4 r = res_get(k);
                    res_put(k, make_float4(fmaf(pend_thr.x, v.x, r.x), fmaf(pend_thr.y, v.y, r.y), fmaf(pend_thr.z, v.z, r.z), 0.f));
                }
            }
            if (last && in_range) {   // the results leave the LDS columns for q.res (what the splat kernels read)
#pragma unroll
                for (int k = 0; k < KMAX; ++k) if (k < rp.n_offsets) q.res[(size_t) k * q.capacity + l] = res_get(k);
            }
        } else if (FIRST) {   // the running result stays in rbase over the inline iterations; every lane's result is defined after the last (nothing zeroed it)
#pragma unroll
            for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) {
                if (commit) rbase[k] = cand[k];
                if (last && in_range && !fuse_splat) q.res[(size_t) k * q.capacity + l] = make_float4(rbase[k].x, rbase[k].y, rbase[k].z, 0.f);
            }
        } else if (commit) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) q.res[(size_t) k * q.capacity + l] = make_float4(cand[k].x, cand[k].y, cand[k].z, 0.f);
        }
        if constexpr (ZROW) if (trace_next) zq_next = zrow_mfma(zrow_m, nra.x, nra.y, nra.z, nrb.x, nrb.y, nrb.z);   // (uniform; as above)
        if (alive && trace_next) {   // closest hit of the continuation ray, consumed by the next bounce (the Hit lives inside this block: no half-defined registers across the commit above)
            Hit h;
            bool found = (F_FLAT || flat) ? trace_flat<false, true, FACTS & kFactsFlatTable, false, ZROW, decltype(zq_next)>(sv, (ConstBytes) A.scene + rp.flat_off, rp.flat_off, flat, stack, mk(nra.x, nra.y, nra.z), mk(nrb.x, nrb.y, nrb.z), nra.w, nrb.w, h, zq_next)
                              : trace_scene<false, MESH, true, RESW != 0, kStackStride, S16, 0u, false, RH16>(sv, stack, mk(nra.x, nra.y, nra.z), mk(nrb.x, nrb.y, nrb.z), nra.w, nrb.w, h);
            if (!FIRST || last) store_hit<MESH>(q, l, h, found);
            if (FIRST) { hh = make_uint4(f2u(h.t), f2u(h.u), f2u(h.v), h.prim); hid = found ? (h.obj | (h.shape << (F_ID24 ? 24u : q.id_shift))) : 0xffffffffu; }
        }
        const uint32_t n_sh = (uint32_t) __popcll(__ballot(want_shadow)) * ((threadIdx.x & 63) == 0 ? 1u : 0u);   // per-wave partial (stats only)
        if (last) n_shadow += n_sh; else if (lane_id == 0) s_inline[2 * it + 1] += n_sh;
    } else {
        uint32_t sslot = seg * kSeg + wave_append(want_shadow, n_shadow);
        if (want_shadow) {
            q.sh_a[sslot] = sha; q.sh_b[sslot] = shb;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets)
                q.sh_c[(size_t) k * q.capacity + sslot] = make_float4(cand[k].x, cand[k].y, cand[k].z, u2f(l));
        }
    }
    if (last) break;
    // next inline iteration: the continuation ray and its closest hit become the lane's current ray (st / stb / stc were set where the
    // bounce computed them); a lane whose path ended sits out the remaining iterations
    lane_on = alive;
    if (alive) { ra = nra; rb = nrb; DTOF_POISON_CHECK(); }
    if constexpr (PAIR) pair_wo = pair_wo_next;
    }   // inline iterations
    if constexpr (!RES_LDS) if (FIRST && fuse_splat) {   // ---- ImageBlock::put (imageblock.cpp:414-531) of the wave's samples: tent filter of radius <= 1, a 3 x 3 footprint anchored at the sample's pixel
        const uint32_t W = (uint32_t) rp.crop_w;
        const uint32_t pix = F_SHIFTS ? (uint32_t) __builtin_amdgcn_readfirstlane((int) (rp.lane_base + l)) >> rp.spp_log2 : fdiv(global_lane<0, false>(rp, rp.lane_base + l), rp.d_spp);   // (as in generate_lane; the fused splat is the float32 film's: no list)
        const int py = (int) fdiv(pix, rp.d_w), px = (int) (pix - W * (uint32_t) py);
        const float sx = pos_reg.x, sy = pos_reg.y;
        const bool regular = in_range && (int) floorf(sx) - rp.crop_x == px && (int) floorf(sy) - rp.crop_y == py;   // (rarely a float position rounds up into the next pixel)
        if (wave_pixel) {   // one pixel per wave: 36 footprint sums over the 64 lanes, lane L < 36 ends up with sum L and adds it to the film
            const int upx = __builtin_amdgcn_readfirstlane(px), upy = __builtin_amdgcn_readfirstlane(py);
            const float relx = (float) (upx + rp.crop_x - 1) + .5f - sx, rely = (float) (upy + rp.crop_y - 1) + .5f - sy;
            float wx[3], wy[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { wx[a] = regular ? tent(relx + (float) a, rp.inv_radius) : 0.f; wy[a] = tent(rely + (float) a, rp.inv_radius); }
            const uint32_t sum_id = __brev(lane_id) >> 26, tap = sum_id >> 2, ch = sum_id & 3u;   // which of the 36 totals this lane ends up with (wave_totals_36)
            const int fx = upx - 1 + (int) (tap % 3u), fy = upy - 1 + (int) (tap / 3u);
            const bool store = sum_id < 36u && (unsigned) fx < W && (unsigned) fy < (unsigned) rp.crop_h;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets) {
                float *fk = A.film + (size_t) k * A.film_stride;
                if (in_range && !regular) splat_lane<F_FUSED_SPLAT ? FILTER_TENT : -1>(rp, fk, sx, sy, px, py, rbase[k].x, rbase[k].y, rbase[k].z);
                float v[36];
#pragma unroll
                for (int ys = 0; ys < 3; ++ys)
#pragma unroll
                    for (int xs = 0; xs < 3; ++xs) {
                        const float w = wx[xs] * wy[ys]; const int c = 4 * (3 * ys + xs);
                        v[c] = rbase[k].x * w; v[c + 1] = rbase[k].y * w; v[c + 2] = rbase[k].z * w; v[c + 3] = w;
                    }
                const float total = wave_totals_36(v, lane_id);
                if (store && total != 0.f) atomicAdd(fk + 4 * ((size_t) fy * W + (size_t) fx) + ch, total);
            }
        } else if (in_range) {   // a ragged chunk: every lane by itself
#pragma unroll
            for (int k = 0; k < KMAX; ++k) if (KMAX == 1 || k < rp.n_offsets)
                splat_lane<F_FUSED_SPLAT ? FILTER_TENT : -1>(rp, A.film + (size_t) k * A.film_stride, sx, sy, px, py, rbase[k].x, rbase[k].y, rbase[k].z);
        }
    }
    }   // chunk loop
    }   // count != 0
    if (lane_id == 0) {
        if (sub > 1) { atomicAdd(&A0.alive_out[seg], n_alive); atomicAdd(&A0.shadow_out[seg], n_shadow); }
        else { A0.alive_out[seg] = n_alive; A0.shadow_out[seg] = n_shadow; }
        if (FIRST) {   // the count slots of the inline iterations before the last lie 2 * n_seg words apart below the last one's (render_rows)
            const uint32_t n_inl = A0.rp.inline_iters, n_seg = RESW ? A0.n_seg : gridDim.x / sub;
            for (uint32_t i = 0; i + 1 < n_inl; ++i) {
                uint32_t *slot = A0.alive_out - (size_t) 2 * (n_inl - 1 - i) * n_seg;
                if (sub > 1) { atomicAdd(&slot[seg], s_inline[2 * i]); atomicAdd(&slot[n_seg + seg], s_inline[2 * i + 1]); }
                else { slot[seg] = s_inline[2 * i]; slot[n_seg + seg] = s_inline[2 * i + 1]; }
            }
        }
    }
    if (!RESW) break;
    }   // segments of a resident wave
#undef DTOF_POISON_CHECK
}

// ---------------------------------------------------------------------------- launch templates (one group of instantiations per dtof_shade_*.hip)
// the six kernels of one (AREA, KMAX, MESH, SPEC) variant: staged / unstaged x split / fused / fused first bounce
template <bool A, int K, bool M, int S>
static void launch_shade_variant(const ShadeLaunch &L) {
#define DTOF_LAUNCH_ONE(LDS_, MODE_) hipLaunchKernelGGL((k_shade<LDS_, MODE_, A, K, M, S>), dim3(L.grid), dim3(kShadeBlock), L.lds, L.stream, L.args)
    if (L.staged) { if (L.mode == 2) DTOF_LAUNCH_ONE(true, 2); else if (L.mode == 1) DTOF_LAUNCH_ONE(true, 1); else DTOF_LAUNCH_ONE(true, 0); }
    else          { if (L.mode == 2) DTOF_LAUNCH_ONE(false, 2); else if (L.mode == 1) DTOF_LAUNCH_ONE(false, 1); else DTOF_LAUNCH_ONE(false, 0); }
#undef DTOF_LAUNCH_ONE
}
// The dynamic LDS of a resident launch lies above the 64 KiB a kernel gets without asking: hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE, so the
// high-water mark of a kernel (or of kernels raised together) is kept per device ordinal (dtof-render drives one host thread per GPU in one process).
static inline void raise_dynamic_lds(std::atomic<uint32_t> (&marks)[64], std::initializer_list<const void *> kernels, uint32_t lds) {
    int dev = 0; (void) hipGetDevice(&dev);
    std::atomic<uint32_t> &mark = marks[(unsigned) dev & 63u]; if (lds <= mark.load()) return;
    for (const void *kernel : kernels)
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess) throw std::runtime_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    mark.store(lds);
}
// the resident form of the fused first-bounce kernel: `waves` waves per block, one block per CU
template <bool A, int K, int S, int W>
static void launch_resident_waves(const ShadeLaunch &L) {
    static std::atomic<uint32_t> attr_lds[64];
    raise_dynamic_lds(attr_lds, { (const void *) k_shade<false, 2, A, K, true, S, W>, (const void *) k_shade<false, 2, A, K, true, S, W, true> }, L.lds);
    if (L.args.rp.res_half) hipLaunchKernelGGL((k_shade<false, 2, A, K, true, S, W, true>), dim3(L.grid), dim3(W * 64), L.lds, L.stream, L.args);   // a TLAS of 1 025 .. 2 048 nodes: half-float planes
    else hipLaunchKernelGGL((k_shade<false, 2, A, K, true, S, W>), dim3(L.grid), dim3(W * 64), L.lds, L.stream, L.args);
}
template <bool A, int K, int S>
static void launch_resident_variant(const ShadeLaunch &L) {
    if (L.waves == 16) launch_resident_waves<A, K, S, 16>(L);
    else if (L.waves == 12) launch_resident_waves<A, K, S, 12>(L);
    else if (L.waves == 8) launch_resident_waves<A, K, S, 8>(L);
    else throw std::runtime_error("resident stage: 8, 12 or 16 waves per block");
}

}  // namespace dtof
