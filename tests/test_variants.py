"""Modulation variants -- (hetero_frequency, hetero_offset) pairs, up to four evaluated in one traversal (dtof_render_variants and the other dtof_*_variants entry
points) -- against the CPU oracle, which is asked once per variant with the integrator's hetero_frequency / hetero_offset set to that pair.

  lanes     every lane of every variant through the BATCHED kernels (Scene.sample_lanes_variants): rgb of variant k as bit patterns, sample_pos / time / ray_o /
            ray_d / valid as well, no lane left out; K = 1 .. 4, both pipelines, one scene per K > 1 kernel family, every waveform with and without the low-pass,
            two time-sampling methods; the same core once more against the pattern-initialised build
  existing  variants at the integrator's own frequency == sample_lanes after set_integrator with each offset, films within IMG_TOL of render(offsets=...)
  films     the developed images of render(variants=...) against the oracle's render / render_exact of each pair
  device    render_rows / render_stripes (and _async) with variants: bands and stripes of 3 ranks == the full frame per plane, the alpha plane at n_variants,
            refusal of a film with too few planes, multi-pass renders
  errors    five variants, the other integrators, null arguments
  velocity  harness.run_scene_velocity_map: one traversal per pass, the wall's -10 m/s"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_TOL = 5e-5     # test_gpu_parity.IMG_TOL: relative to max|ref|; the lanes are bit-exact, only the float32 order of the film sums differs
PX_TOL = 1e-3      # test_gpu_parity.PX_TOL: per-pixel relative L-inf against the order-independent film (render_exact)
NCPU = min(os.cpu_count() or 1, 16)

# the four films of harness.calc_velocity_from_homo_heteros: homodyne and heterodyne at two offsets
SET_K4 = [(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]
SET_K2 = [(0.3, 0.1), (-0.7, 0.9)]                    # frequencies float32 cannot represent, one of them negative
SET_K3 = [(2.5, 0.5), (0.0, 0.125), (-1.0, 0.7)]
SET_K1 = [(0.37, 0.6)]                               # one film, at a frequency other than the scene's
SETS = {"k4": SET_K4, "k2": SET_K2, "k3": SET_K3, "k1": SET_K1}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rel_linf(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def rel_linf_px(a, ref, eps=1e-3):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    floor = eps * max(np.abs(ref).max(), 1e-30)
    return float((np.abs(a - ref) / np.maximum(np.abs(ref), floor)).max())


def integrator_of(osc, **override):
    """the scene file's integrator as the dictionary Scene.params(integrator=...) takes, with properties replaced"""
    ip = osc.flat.integrator
    conv = {"float": float, "int": int, "bool": bool}
    d = {"type": ip.plugin}
    d.update({k: conv.get(t, str)(v) for k, (t, v) in ip.items()})
    d.update(override)
    return d


def oracle_lanes(osc, base, variant, seed, spp, begin, n):
    f, o = variant
    pd = osc.params(integrator=dict(base, hetero_frequency=float(np.float32(f)), hetero_offset=float(np.float32(o))))
    return osc.render_lanes(pd, seed, spp, begin, n, threads=NCPU)


def check_lanes(mi, orc, path, params, spp, variants, integrator=None, seed=2, what=""):
    """every lane of the frame, every variant, against the oracle; returns the GPU lanes"""
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    base = integrator if integrator is not None else integrator_of(osc)
    if integrator is not None:
        sc.set_integrator(integrator)
    w, h = sc.size
    n = w * h * spp
    g = sc.sample_lanes_variants(seed, spp, 0, n, variants)
    assert g["rgb"].shape == (len(variants), n, 3)
    lit = 0
    for k, v in enumerate(variants):
        o = oracle_lanes(osc, base, v, seed, spp, 0, n)
        for f in ("sample_pos", "time", "ray_o", "ray_d"):
            assert np.array_equal(bits(g[f]), bits(o[f])), (what, v, f, int((bits(g[f]) != bits(o[f])).sum()))
        assert np.array_equal(g["valid"], o["valid"]), (what, v, "valid", int((g["valid"] != o["valid"]).sum()))
        bad = (bits(g["rgb"][k]) != bits(o["rgb"])).any(axis=1)
        assert not bad.any(), (what, "variant %d %s" % (k, (v,)), "%d of %d lanes differ" % (int(bad.sum()), n))
        lit += int((o["rgb"] != 0).any(axis=1).sum())
    assert lit > 0, what      # the films are not all black
    return sc, g


def resident(waves):
    """the switches with which the existing Domino tests turn the resident first-bounce stage on for a small frame"""
    return dict(DTOF_PIPELINE="fused", DTOF_CHUNK_SEGS="0", DTOF_RESIDENT=str(waves))


FUSED, SPLIT = dict(DTOF_PIPELINE="fused"), dict(DTOF_PIPELINE="split")


def _mesh_blas(tmp):
    """the room of test_meshes.py: a static ply and a moving obj mesh, each behind its own BLAS (the ray kernels run as a pair of launches)"""
    sys.path.insert(0, SCENES)
    import make_mesh
    make_mesh.write_all(tmp, 24, 12)
    path = os.path.join(tmp, "cornell_mesh.xml")
    open(path, "w").write(make_mesh.cornell_mesh_xml())
    return path


# one scene per K > 1 kernel family: (scene file or None for the BLAS room, -D parameters, spp, environment settings)
SCENE_CASES = {
    "wall": ("cornell_wall.xml", dict(resx=24, resy=16), 8, (FUSED, SPLIT)),                       # the moving wall: plain kernels, instance memo
    "boxes": ("cornell_boxes.xml", dict(resx=24, resy=16), 8, (FUSED, SPLIT)),                     # mesh kernels
    "area": ("cornell_area.xml", dict(resx=24, resy=16, max_depth=5), 8, (FUSED, SPLIT)),          # the emitter-hit term
    "spec1": ("cornell_roughplastic.xml", dict(resx=24, resy=16, max_depth=5), 8, (FUSED, SPLIT)), # every-BSDF kernels
    "spec2": ("cornell_blend.xml", dict(resx=24, resy=16, max_depth=6), 8, (FUSED, SPLIT)),        # ... with blendbsdf
    "mesh_blas": (None, dict(resx=24, resy=16), 4, ({}, FUSED, SPLIT)),                            # ray kernels as a pair of launches
    "domino_resident": ("domino.xml", dict(resx=48, resy=32), 4, (resident(8), resident(16))),     # the resident several-film kernel (results in LDS)
    "rgba_open": ("open_veils.xml", dict(resx=24, resy=16, max_depth=5, pixel_format="rgba"), 8, (FUSED, SPLIT)),   # valid flags of an open scene
}
LANE_CASES = [(name, s) for name, c in SCENE_CASES.items() for s in range(len(c[3]))]


def _env_id(env):
    return "default" if not env else env["DTOF_PIPELINE"] + ("_res" + env["DTOF_RESIDENT"] if "DTOF_RESIDENT" in env else "")


@pytest.mark.parametrize("case", LANE_CASES, ids=lambda c: c[0] + "-" + _env_id(SCENE_CASES[c[0]][3][c[1]]))
def test_lanes_core_every_kernel_family_four_variants(mi, orc, case, monkeypatch, tmp_path):
    name, s = case
    xml, params, spp, envs = SCENE_CASES[name]
    for k, v in envs[s].items():
        monkeypatch.setenv(k, v)
    path = _mesh_blas(str(tmp_path)) if xml is None else os.path.join(SCENES, xml)
    sc, g = check_lanes(mi, orc, path, params, spp, SET_K4, what=name)
    if name == "rgba_open":
        assert sc.info()["has_alpha"] and 0 < int(g["valid"].sum()) < g["valid"].size     # the flags carry information
    if name == "domino_resident":
        assert sc.info()["n_objects"] == 1025


@pytest.mark.parametrize("pipeline", ["fused", "split"])
@pytest.mark.parametrize("vset", ["k2", "k3", "k1"])
@pytest.mark.parametrize("scene", ["cornell_wall.xml", "cornell_area.xml"])
def test_lanes_core_other_variant_counts(mi, orc, scene, vset, pipeline, monkeypatch):
    monkeypatch.setenv("DTOF_PIPELINE", pipeline)
    check_lanes(mi, orc, os.path.join(SCENES, scene), dict(resx=24, resy=16), 8, SETS[vset], what=(scene, vset, pipeline))


@pytest.mark.parametrize("pipeline", ["fused", "split"])
@pytest.mark.parametrize("tsm", ["antithetic", "stratified"])
@pytest.mark.parametrize("low_pass", [True, False])
@pytest.mark.parametrize("wave", ["sinusoidal", "rectangular", "triangular", "trapezoidal"])
def test_lanes_core_modulation_settings(mi, orc, wave, low_pass, tsm, pipeline, monkeypatch):
    """every waveform in the low-pass and the full modulation ((w_g + w_d) * t + phase is formed per film there), two time-sampling methods; the integrator carries
    a frequency and an offset of its own that no variant repeats"""
    monkeypatch.setenv("DTOF_PIPELINE", pipeline)
    integ = dict(type="dopplertofpath", max_depth=4, w_g=30.0, hetero_frequency=1.0, hetero_offset=0.4, path_correlation_depth=4, time_sampling_method=tsm,
                 antithetic_shift=0.5 if tsm == "antithetic" else 0.0, wave_function_type=wave, low_frequency_component_only=low_pass)
    for vset in ("k4", "k2"):
        check_lanes(mi, orc, os.path.join(SCENES, "cornell_wall.xml"), dict(resx=16, resy=16), 8, SETS[vset], integrator=integ, what=(wave, low_pass, tsm, pipeline, vset))


def test_lanes_core_on_the_pattern_initialised_build():
    """the lane tests above in a child process whose library starts every uninitialised automatic variable as a NaN pattern (the K = 4 kernels have a history there,
    profiles/r03_k4_uninitialised.txt), the way tests/test_pattern_build.py runs the parity tests"""
    lib = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_pattern.so")
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(lib):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "lanes_core and not pattern"],
                       env=dict(os.environ, DTOF_LIB=lib), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]


# ---------------------------------------------------------------- what exists already
@pytest.mark.parametrize("pipeline", ["fused", "split"])
def test_variants_at_the_integrators_frequency_are_the_offsets(mi, orc, pipeline, monkeypatch):
    monkeypatch.setenv("DTOF_PIPELINE", pipeline)
    path, params, spp = os.path.join(SCENES, "cornell_boxes.xml"), dict(resx=24, resy=16, wave_function_type="trapezoidal"), 8
    offs = [0.0, 0.25, 0.5, 0.75]
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    f0 = sc.info()["hetero_frequency"]
    variants = [(f0, o) for o in offs]
    n = 24 * 16 * spp
    g = sc.sample_lanes_variants(3, spp, 0, n, variants)
    films = sc.render(seed=3, spp=spp, variants=variants)
    ref = sc.render(seed=3, spp=spp, offsets=offs)
    for k, o in enumerate(offs):
        one = mi.load_file(path, **params)
        one.set_integrator(integrator_of(osc, hetero_offset=o))     # the scene file's integrator with this offset
        sc_k = one.sample_lanes(3, spp, 0, n)
        for f in ("sample_pos", "time", "ray_o", "ray_d"):
            assert np.array_equal(bits(g[f]), bits(sc_k[f])), (o, f)
        assert np.array_equal(bits(g["rgb"][k]), bits(sc_k["rgb"])), (o, int((bits(g["rgb"][k]) != bits(sc_k["rgb"])).any(axis=1).sum()))
        assert np.array_equal(g["valid"], sc_k["valid"])
        assert rel_linf(films[k], ref[k]) <= IMG_TOL, (o, rel_linf(films[k], ref[k]))
    # no variants: the integrator's own pair, one plane
    own = sc.sample_lanes_variants(3, spp, 0, n)
    plain = sc.sample_lanes(3, spp, 0, n)
    assert own["rgb"].shape == (1, n, 3) and np.array_equal(bits(own["rgb"][0]), bits(plain["rgb"]))


# ---------------------------------------------------------------- films
def test_films_of_render_variants_match_the_oracle(mi, orc):
    """the inputs on which test_gpu_parity.test_batched_offsets_equal_separate_renders holds the offset batch to these criteria; a list longer than four is grouped"""
    path, params = os.path.join(SCENES, "cornell_boxes.xml"), dict(resx=32, resy=32, wave_function_type="trapezoidal")
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    variants = SET_K4 + SET_K2
    films = sc.render(seed=2, spp=16, variants=variants)
    assert films.shape == (6, 32, 32, 3)
    assert sc.last_stats["n_paths"] == 2 * 32 * 32 * 16        # two traversals for six films
    four = sc.render(seed=2, spp=16, variants=SET_K4)
    assert sc.last_stats["n_paths"] == 32 * 32 * 16            # one traversal for four films
    assert rel_linf(four, films[:4]) <= IMG_TOL                # (two renders of one film differ in the order of their float32 film sums)
    for k, (f, o) in enumerate(variants):
        pd = osc.params(integrator=integrator_of(osc, hetero_frequency=float(np.float32(f)), hetero_offset=float(np.float32(o))))
        ref, _ = osc.render(pd, seed=2, spp=16, threads=NCPU)
        exact, _ = osc.render_exact(pd, seed=2, spp=16, threads=NCPU)
        e, e_px = rel_linf(films[k], ref), rel_linf_px(films[k], exact)
        print("variant", (f, o), "rel_linf", e, "rel_linf_px", e_px)
        assert e <= IMG_TOL, ((f, o), e)
        assert e_px <= PX_TOL, ((f, o), e_px)
    integ = mi.load_dict(integrator_of(osc))
    assert rel_linf(integ.render(sc, seed=2, spp=16, variants=SET_K4), four) <= IMG_TOL


# ---------------------------------------------------------------- device films
def _planes(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("scene,params,spp", [("cornell_wall.xml", dict(resx=32, resy=24), 8),
                                              ("open_veils.xml", dict(resx=32, resy=24, max_depth=5, pixel_format="rgba"), 8)], ids=["rgb", "rgba"])
def test_device_films_bands_stripes_async_and_the_alpha_plane(mi, orc, scene, params, spp):
    import torch
    from mitsuba3dopplertof_amd import distributed as D
    path = os.path.join(SCENES, scene)
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    W, H = sc.size
    alpha = bool(sc.info()["has_alpha"])
    K, world, seed = 4, 3, 5
    planes = sc.film_planes(K)
    assert planes == K + (1 if alpha else 0)

    def new_film():
        t = torch.zeros((planes, H, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        return t
    if alpha:   # refused until the film is declared, and with too few planes; nothing is written
        film = new_film()
        with pytest.raises(mi.DtofError, match="dtof_scene_set_film_layout"):
            sc.render_rows(film.data_ptr(), seed, spp, 0, H, variants=SET_K4)
        sc.set_film_layout(K)
        with pytest.raises(mi.DtofError, match="needs 5 RGBW planes"):
            sc.render_rows(film.data_ptr(), seed, spp, 0, H, variants=SET_K4)
        with pytest.raises(mi.DtofError, match="needs 5 RGBW planes"):
            sc.render_stripes(film.data_ptr(), seed, spp, 0, 4, 12, variants=SET_K4)
        assert float(np.abs(_planes(film)).sum()) == 0.0
        sc.set_film_layout(planes)
    else:
        film = new_film()
        sc.set_film_layout(2)
        with pytest.raises(mi.DtofError, match="declared with 2 planes, this call writes 4"):
            sc.render_rows(film.data_ptr(), seed, spp, 0, H, variants=SET_K4)
        with pytest.raises(mi.DtofError, match="declared with 2 planes, this call writes 3"):
            sc.render_stripes_async(film.data_ptr(), seed, spp, 0, 4, 12, variants=SET_K3)
        assert float(np.abs(_planes(film)).sum()) == 0.0
        sc.set_film_layout(0)
    full = new_film()
    st_full = sc.render_rows(full.data_ptr(), seed, spp, 0, H, variants=SET_K4)
    assert st_full["n_paths"] == W * H * spp
    full_h = _planes(full)
    # plane k is the oracle's film of variant k, the alpha film is plane K
    for k, (f, o) in enumerate(SET_K4):
        pd = osc.params(integrator=integrator_of(osc, hetero_frequency=float(np.float32(f)), hetero_offset=float(np.float32(o))))
        raw, _ = osc.render(pd, seed=seed, spp=spp, raw=True, threads=NCPU)
        assert rel_linf(full_h[k][..., :3], raw[..., :3]) <= IMG_TOL, (k, rel_linf(full_h[k][..., :3], raw[..., :3]))
        assert rel_linf(full_h[k][..., 3], raw[..., 3]) <= IMG_TOL
    if alpha:
        a = osc.render_alpha(osc.params(), seed=seed, spp=spp, threads=NCPU)
        dev = full_h[K][..., 0] / np.where(full_h[K][..., 3] == 0, 1, full_h[K][..., 3])
        assert np.abs(dev - a).max() <= 1e-5 and 0.05 < a.mean() < 0.999
        assert np.array_equal(full_h[K][..., 1:3], np.zeros_like(full_h[K][..., 1:3]))
    # bands of three ranks, synchronous and asynchronous
    for use_async in (False, True):
        union, lanes = new_film(), 0
        for r in range(world):
            r0, r1 = D.row_band(H, world, r)
            if use_async:
                sc.render_rows_async(union.data_ptr(), seed, spp, r0, r1, variants=SET_K4)
            else:
                lanes += sc.render_rows(union.data_ptr(), seed, spp, r0, r1, variants=SET_K4)["n_paths"]
        if use_async:
            lanes = sc.collect()[0]["n_paths"]
        assert lanes == W * H * spp
        u = _planes(union)
        for p in range(planes):
            assert rel_linf(u[p], full_h[p]) <= IMG_TOL, ("bands", use_async, p, rel_linf(u[p], full_h[p]))
    # stripes of three ranks with a height that does not divide the frame, K = 3 as well
    for variants in (SET_K4, SET_K3):
        k = len(variants)
        ref = new_film()
        sc.set_film_layout(planes)
        sc.render_rows(ref.data_ptr(), seed, spp, 0, H, variants=variants)
        ref_h = _planes(ref)
        for use_async in (False, True):
            union = new_film()
            for r in range(world):
                layout = D.stripe_layout(world, r, 5)
                if use_async:
                    sc.render_stripes_async(union.data_ptr(), seed, spp, *layout, variants=variants)
                else:
                    sc.render_stripes(union.data_ptr(), seed, spp, *layout, variants=variants)
            if use_async:
                assert sc.collect()[0]["n_paths"] == W * H * spp
            u = _planes(union)
            for p in range(k + (1 if alpha else 0)):
                assert rel_linf(u[p], ref_h[p]) <= IMG_TOL, ("stripes", k, use_async, p)
            assert float(np.abs(u[k + (1 if alpha else 0):]).sum()) == 0.0      # the planes behind the call's own stay untouched
            if alpha and k == 3:
                assert rel_linf(u[3], full_h[4]) <= IMG_TOL                      # the alpha film moved to plane n_variants = 3
    sc.set_film_layout(0)


def test_multi_pass_render_with_variants_matches_the_oracle(mi, orc):
    """samples_per_pass: the streams run on from pass to pass; every (pass, lane) of every variant, and the accumulated films"""
    path, params = os.path.join(SCENES, "cornell_area.xml"), dict(resx=24, resy=16)
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    spp, per_pass = 8, 2
    multi = dict(type="dopplertofpath", max_depth=4, path_correlation_depth=2, time_sampling_method="antithetic", hetero_frequency=1.0, samples_per_pass=per_pass)
    sc.set_integrator(multi)
    wavefront = 24 * 16 * per_pass
    for p in range(spp // per_pass):
        g = sc.sample_lanes_variants(4, spp, p * wavefront, wavefront, SET_K4)
        for k, v in enumerate(SET_K4):
            o = oracle_lanes(osc, multi, v, 4, spp, p * wavefront, wavefront)
            for f in ("sample_pos", "time", "ray_d"):
                assert np.array_equal(bits(g[f]), bits(o[f])), ("pass", p, v, f)
            assert np.array_equal(bits(g["rgb"][k]), bits(o["rgb"])), ("pass", p, v, int((bits(g["rgb"][k]) != bits(o["rgb"])).any(axis=1).sum()))
    films = sc.render(seed=4, spp=spp, variants=SET_K4)
    assert sc.last_stats["n_paths"] == 24 * 16 * spp
    for k, (f, o) in enumerate(SET_K4):
        ref, _ = osc.render(osc.params(integrator=dict(multi, hetero_frequency=f, hetero_offset=o)), seed=4, spp=spp, threads=NCPU)
        assert rel_linf(films[k], ref) <= IMG_TOL, ((f, o), rel_linf(films[k], ref))


# ---------------------------------------------------------------- errors
def test_errors_of_the_variants_entry_points(mi):
    import torch
    L = mi._lib()
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=16, resy=16)
    five = np.ascontiguousarray([(0.0, 0.1 * i) for i in range(5)], np.float32)
    one = np.ascontiguousarray([(1.0, 0.0)], np.float32)
    film = torch.zeros((5, 16, 16, 4), dtype=torch.float32, device="cuda")
    out, lanes, rgb = np.zeros((5, 16, 16, 3), np.float32), np.zeros((64, 12), np.float32), np.zeros((5, 64, 3), np.float32)
    st = mi._Stats()
    INVALID = 1

    def calls(var, n):
        v = var.ctypes.data if var is not None else None
        return {"render": lambda: L.dtof_render_variants(sc._h, 0, 4, v, n, out.ctypes.data, C.byref(st)),
                "rows": lambda: L.dtof_render_rows_variants(sc._h, 0, 4, 0, 16, v, n, film.data_ptr(), C.byref(st)),
                "rows_async": lambda: L.dtof_render_rows_variants_async(sc._h, 0, 4, 0, 16, v, n, film.data_ptr()),
                "stripes": lambda: L.dtof_render_stripes_variants(sc._h, 0, 4, 0, 4, 8, v, n, film.data_ptr(), C.byref(st)),
                "stripes_async": lambda: L.dtof_render_stripes_variants_async(sc._h, 0, 4, 0, 4, 8, v, n, film.data_ptr()),
                "lanes": lambda: L.dtof_sample_lanes_variants(sc._h, 0, 4, v, n, 0, 64, lanes.ctypes.data, None, rgb.ctypes.data)}
    for name, call in calls(five, 5).items():
        assert call() == INVALID, name
        assert b"at most 4 modulation variants" in L.dtof_last_error(), (name, L.dtof_last_error())
    for plugin in ("path", "velocity"):
        sc.set_integrator(dict(type=plugin))
        for name, call in calls(one, 1).items():
            assert call() == INVALID, (plugin, name)
            assert L.dtof_last_error() == b"modulation offsets only apply to the dopplertofpath integrator", (plugin, name, L.dtof_last_error())
        for name, call in calls(None, 0).items():      # no variants: the integrator's own render
            assert call() == 0, (plugin, name, L.dtof_last_error())
        sc.collect()
    torch.cuda.synchronize()
    sc.set_integrator(dict(type="dopplertofpath"))
    film.zero_()
    torch.cuda.synchronize()
    v = one.ctypes.data
    assert L.dtof_render_variants(None, 0, 4, v, 1, out.ctypes.data, C.byref(st)) == INVALID
    assert L.dtof_render_variants(sc._h, 0, 4, v, 1, None, C.byref(st)) == INVALID
    assert L.dtof_render_rows_variants(sc._h, 0, 4, 0, 16, v, 1, None, C.byref(st)) == INVALID
    assert L.dtof_render_rows_variants(None, 0, 4, 0, 16, v, 1, film.data_ptr(), C.byref(st)) == INVALID
    assert L.dtof_render_rows_variants_async(sc._h, 0, 4, 0, 16, v, 1, None) == INVALID
    assert L.dtof_render_stripes_variants(sc._h, 0, 4, 0, 4, 8, v, 1, None, C.byref(st)) == INVALID
    assert L.dtof_render_stripes_variants_async(None, 0, 4, 0, 4, 8, v, 1, film.data_ptr()) == INVALID
    assert L.dtof_sample_lanes_variants(sc._h, 0, 4, v, 1, 0, 64, None, None, rgb.ctypes.data) == INVALID
    assert L.dtof_sample_lanes_variants(sc._h, 0, 4, v, 1, 0, 64, lanes.ctypes.data, None, None) == INVALID
    assert L.dtof_sample_lanes_variants(None, 0, 4, v, 1, 0, 64, lanes.ctypes.data, None, rgb.ctypes.data) == INVALID
    assert b"null argument" in L.dtof_last_error()
    torch.cuda.synchronize()
    assert float(film.abs().sum()) == 0.0          # none of the refused calls wrote
    with pytest.raises(mi.DtofError, match="either offsets or variants"):
        sc.render(seed=0, spp=4, offsets=[0.0], variants=[(1.0, 0.0)])


# ---------------------------------------------------------------- the velocity map
def test_velocity_map_from_one_traversal_per_pass(mi):
    """the inputs of the two-render test of tests/test_io_and_harness.py: the wall moves at -10 m/s"""
    from mitsuba3dopplertof_amd import harness
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=32, resy=32)
    v, films = harness.run_scene_velocity_map(sc, total_spp=4096, time_sampling_method="antithetic", path_correlation_depth=16, max_depth=2)
    assert v.shape == (32, 32) and len(films["homodyne"]) == 2 and len(films["heterodyne"]) == 2
    centre = v[12:20, 12:20]
    print("median of the centre 8x8:", float(np.median(centre)))
    assert abs(np.median(centre) + 10.0) < 2.5, np.median(centre)
    # 4096 samples = 4 passes of 1024: one traversal each, whatever the number of films
    assert len(sc.pass_stats) == 4
    for st in sc.pass_stats:
        assert st["n_paths"] == 32 * 32 * 1024, st["n_paths"]
    # the homodyne film of offset 0 is the plain harness render of that integrator
    one = harness.run_scene_doppler_tof(sc, total_spp=1024, hetero_frequency=0.0, hetero_offset=0.0, time_sampling_method="antithetic", path_correlation_depth=16, max_depth=2)
    batch = harness.run_scene_doppler_tof_variants(sc, [(0.0, 0.0), (1.0, 0.25)], total_spp=1024, time_sampling_method="antithetic", path_correlation_depth=16, max_depth=2)
    assert rel_linf(batch[0], one) <= IMG_TOL
