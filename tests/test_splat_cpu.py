"""The criterion the float32 splat kernels are held to (tests/splat_ref.py: |film - E| <= (n + 2) 2^-24 M per pixel and channel) is neither vacuous nor wrong, shown
without a device on every case of tests/splat_cases.py:

  - the oracle's own raw float32 film (orc.Scene.render(raw=True): the same terms added in float32, serially per band of rows) lies within the bound of E: an
    independent float32 summation passes;
  - a lane lost or counted twice is seen.  Either moves the pixels of its footprint by exactly its terms, so splat_ref.loss_seen answers for EVERY lane at once: all
    of them at every sample count up to 512; at 1024 spp (n = 9216 terms a pixel, a bound of 0.56 on the weight channel) the samples within about a quarter pixel of
    a pixel centre, most of them.  The helpers that perturb a copy of the lane set -- drop_lane, double_lane, swap_channels, shift_row, misplace_irregular -- are
    each flagged in at least one pixel on every case they apply to;
  - the irregular-sample frames hold irregular samples: at least 8 lanes per axis whose float position floors into the next pixel, some in the window's last column
    or row, at the sample count each kernel family runs them with.  Misplacing one (its weights one pixel off) is flagged; evaluating its weights again for the
    nominal anchor -- a kernel without a path of its own for such samples -- gives THE SAME FILM, so no criterion can tell that apart, and none needs to;
  - the choice of the kernel (csrc/dtof_splat_choice.h) tabulated on the host by tests/splat_choice_check.cpp: its properties hold over the whole table, the named
    requests give the kernels and shapes the cases expect, and launch_splat launches nothing the function did not choose."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_ref as aref
import moments_ref as ref
import splat_cases as cases
import splat_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = [name for name, c in cases.CASES.items() if c["frame"].startswith("far")]
_cache = {}


def prepared(orc, name):
    """(case, oracle scene, Lanes, LaneSet, E, M, n), computed once per scene and sample count"""
    c = cases.CASES[name]
    key = (c["filter"], c["frame"], c["spp"], c["K"], c["rgba"], c["rows"])
    if key not in _cache:
        xml, params = cases.scene_xml(c)
        osc = orc.Scene(xml, params, is_string=True)
        lanes = aref.Lanes(orc, osc, cases.SEED, c["spp"], cases.variants(c))
        ls = sref.LaneSet.of(lanes, alpha=c["rgba"], rows=c["rows"])
        _cache[key] = (osc, lanes, ls) + sref.film(ls)
    return (c,) + _cache[key]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_oracles_float32_film_lies_within_the_bound(orc, name):
    c, osc, lanes, ls, E, M, n = prepared(orc, name)
    variants = cases.variants(c) or [None]
    assert E.shape == (len(variants) + c["rgba"],) + osc.size[::-1] + (4,) and n.max() <= 25 * 1024
    for k, v in enumerate(variants):
        pd = osc.params() if v is None else osc.params(integrator=ref.integrator_of(osc, hetero_frequency=float(ref.F32(v[0])), hetero_offset=float(ref.F32(v[1]))))
        raw = osc.render(pd, seed=cases.SEED, spp=c["spp"], raw=True, rows=c["rows"], threads=ref.NCPU)[0]
        ratios = sref.errors_over_bound(raw[None], E[k:k + 1], M[k:k + 1], n)
        print("%s plane %d: oracle float32 film, largest error / bound (r g b w): %s" % (name, k, " ".join("%.3g" % r for r in ratios[0])))
        assert np.abs(raw[..., :3]).max() > 0 and (ratios <= 1.0).all(), (name, k, ratios)
    r0, r1 = c["rows"] or (0, osc.size[1])
    assert (M[:, r0:r1, :, 3] > 0).all() and (M.reshape(len(M), osc.size[1], -1)[:, :max(r0 - 3, 0)] == 0).all()      # every rendered pixel has weight; rows far above a band have nothing
    if c["rgba"]:
        assert E[-1][..., 0].max() > 0 and not E[-1][..., 1:3].any()      # the alpha plane is (A, 0, 0, W)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_mutation_is_flagged(orc, name):
    c, osc, lanes, ls, E, M, n = prepared(orc, name)
    live = ls.inside.any(axis=1)
    seen = sref.loss_seen(ls, M, n)[live]
    print("%s: a lost or doubled lane is seen for %d of %d lanes" % (name, seen.sum(), len(seen)))
    if c["spp"] <= 512:
        assert seen.all(), (name, int((~seen).sum()))
    else:      # 1024 spp: (9 * 1024 + 2) 2^-24 * M_W with M_W about 1024 is 0.56 -- the tent's weight exceeds it within about a quarter pixel of the centre
        assert seen.mean() > 0.5, (name, seen.mean())
    i = sref.interior_lane(ls)
    for what, mutate in (("drop_lane", sref.drop_lane), ("double_lane", sref.double_lane), ("swap_channels", sref.swap_channels), ("shift_row", sref.shift_row)):
        assert sref.flagged(mutate(ls, i), E, M, n) > 0, (name, what, i)
    assert sref.flagged(ls, E, M, n) == 0      # and the unperturbed set is not


@pytest.mark.parametrize("name", FAR)
def test_the_irregular_sample_frames(orc, name):
    c, osc, lanes, ls, E, M, n = prepared(orc, name)
    W, H = osc.size
    ix, iy = ls.irregular()
    px, py = ls.nominal()
    last = int((ix & (px == W - 1)).sum() + (iy & (py == H - 1)).sum())
    print("%s: %d lanes floor into the next pixel along x, %d along y, %d of them in the last column or row" % (name, ix.sum(), iy.sum(), last))
    assert ix.sum() >= cases.FAR_MIN and iy.sum() >= cases.FAR_MIN and last >= 1, (name, ix.sum(), iy.sum(), last)
    # such a position IS the next integer, and only one pixel off
    for axis, mask, nominal in ((0, ix, px), (1, iy, py)):
        p = ls.pos[mask, axis].astype(np.float64) - float(osc.flat.sensor[("crop_x", "crop_y")[axis]])
        assert (p == nominal[mask] + 1).all(), (name, axis)
    both = np.flatnonzero(ix | iy)
    seen = sref.loss_seen(ls, M, n)
    assert seen[both].all(), name      # an irregular lane splatted by neither path, or by both
    for i in both:
        assert sref.flagged(sref.misplace_irregular(ls, orc, int(i)), E, M, n) > 0, (name, int(i))
        same = sref.film(sref.misplace_irregular(ls, orc, int(i), reweigh=True))[0]
        assert (np.abs(same - E) <= 2.0 ** -45 * M).all(), (name, int(i))      # the same terms: two float64 orders of them at most


def test_the_choice_table(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc")
    exe = str(tmp_path / "splat_choice_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", src, os.path.join(ROOT, "tests", "splat_choice_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "FAIL|" not in out.stdout, out.stdout[-3000:]
    got = dict(ln.split("|", 1) for ln in out.stdout.splitlines())
    assert int(got["entries"]) > 900000 and all(int(got["count " + k]) > 0 for k in ("generic", "tent3", "x8", "pixel")) and got["count none"] == got["count fused"] == "0"
    # name -> kernel n seg parts chunk lds word
    want = {"tent@16": "x8 3 2 0 0 18432 0x9b", "tent@64": "x8 3 8 0 0 4608 0x19b", "tent@512": "x8 3 64 0 0 576 0x31b", "tent@1024": "x8 3 64 0 0 576 0x31b",
            "box@128": "x8 1 16 0 0 256 0x20b", "gaussian stddev .25@32": "x8 3 4 0 0 9216 0x11b", "gaussian@16": "x8 5 2 0 0 51200 0xab",
            "tent 2.5@16": "x8 5 2 0 0 51200 0xab", "tent 2.6@16": "generic 7 0 0 0 0 0x39", "tent .5@16": "generic 1 0 0 0 0 0x9", "lanczos@16": "generic 7 0 0 0 0 0x39",
            "tent@1": "pixel 3 0 1 1 0 0x101c", "tent@2": "tent3 3 2 0 0 0 0x9a", "tent@8": "tent3 3 8 0 0 0 0x19a", "tent@3": "pixel 3 0 1 3 0 0x301c",
            "tent@12": "pixel 3 0 1 12 0 0xc01c", "tent@17": "pixel 3 0 2 9 0 0x909c", "tent@24": "pixel 3 0 2 12 0 0xc09c", "tent@33": "pixel 3 0 4 9 0 0x911c",
            "tent@100": "pixel 3 0 8 13 0 0xd19c", "gaussian@4": "pixel 5 0 1 4 0 0x402c", "tent@48 full frame": "pixel 3 0 1 48 0 0x3001c",
            "tent@16 generic": "generic 3 0 0 0 0 0x19", "tent@16 dpp": "tent3 3 16 0 0 0 0x21a", "gaussian@16 dpp": "generic 5 0 0 0 0 0x29"}
    assert {k: v for k, v in got.items() if k != "entries" and not k.startswith("count ")} == want
    # launch_splat asks this function and launches what it says: no condition of its own on the filter's radius, the sample count or the switch
    kernels = open(os.path.join(src, "dtof_kernels.hip")).read()
    body = kernels[kernels.index("uint32_t launch_splat("):kernels.index("__global__ void k_pass_save(")]
    assert "splat_choice(f)" in body and "return c.packed();" in body
    assert not re.search(r"filter_radius\s*[<>]|rp\.spp\s*[<>]|spp_log2\s*[!=]=|ls\.splat\s*[!=]=|ceilf", body)
    for field in ("filter", "radius", "spp", "spp_log2", "n_lanes", "splat_switch"):
        assert "f.%s = " % field in body, field
    render = open(os.path.join(src, "dtof_render.hip")).read()
    assert "sc->last_splat = launch_splat(" in render and "sc->last_splat = kSplatFusedWord" in render


def test_the_python_property_unpacks_the_word(mi):
    """Scene.last_splat against the packed words of the table above (no device: the entry is driven through a stand-in handle's word)"""
    class Lib:
        def __init__(self, w):
            self.w = w

        def dtof_scene_last_splat(self, h):
            return self.w
    sc = object.__new__(mi.Scene)
    sc._h = None
    real = mi._abi._lib
    try:
        for word, want in ((0x9b, cases.x8(3, 2)), (0x31b, cases.x8(3, 64)), (0xd19c, cases.pixel(3, 8, 13)), (0x19a, cases.tent3(8)), (0x39, cases.generic(7)),
                           (5 | (3 << 3), cases.FUSED), (0, None)):
            mi._abi._lib = lambda w=word: Lib(w)
            assert sc.last_splat == want, (hex(word), sc.last_splat)
    finally:
        mi._abi._lib = real
        sc._h = None
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    assert re.search(r"\buint32_t\s+dtof_scene_last_splat\s*\(const dtof_scene \*scene\)\s*;", hdr)
