"""The inputs of the BSDF sweep (tests/bsdf_sweep.py), judged by the oracle alone: that the array entry orc_kat_bsdf_n is orc_kat_bsdf, that family C really
lands ON the thresholds of the lobe choices and that the lobe changes across them, that every material meets the operand classes the families name, and that
NaN rows stay a small share (two NaNs compare equal in test_bsdf_sweep_gpu.py, so they must not become most of the comparison).  The device leg is
test_bsdf_sweep_gpu.py: it runs these very queries through every instantiation of the shade kernels' BSDF function."""
import ctypes as C

import numpy as np
import pytest

import bsdf_sweep as bs

@pytest.fixture(scope="module")
def texdir(tmp_path_factory):
    return bs.write_textures(tmp_path_factory.mktemp("bsdf_sweep"))


@pytest.fixture(scope="module")
def swept(orc, texdir):
    """name -> (material, {family: queries}, {family: oracle outputs (n, 17)}, family C's bookkeeping); the last material is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            m = {x.name: x for x in bs.catalogue(texdir)}[name]
            osc = orc.Scene(bs.SCENE % m.bsdf, {}, is_string=True)
            ev = lambda q: bs.oracle_eval(orc, osc.c.shapes[0], q)   # noqa: E731
            fam, c = bs.families(m, ev)
            cache[name] = (m, fam, {k: ev(q) for k, q in fam.items()}, c, osc)
        return cache[name][:4]
    return get


@pytest.mark.parametrize("name", bs.NAMES)
def test_array_entry_is_the_scalar_entry(orc, texdir, name):
    """orc_kat_bsdf_n on the flat frame at uv = 0 equals orc_kat_bsdf bit for bit: 10^4 queries per material, half random, half from the edge grid"""
    m = {x.name: x for x in bs.catalogue(texdir)}[name]
    osc = orc.Scene(bs.SCENE % m.bsdf, {}, is_string=True)
    shape, L = osc.c.shapes[0], orc.lib()
    b = bs.family_b()
    q = np.concatenate([bs.family_a(5000), b[::len(b) // 5000][:5000]])
    q[:, 9:11] = 0
    got = bs.oracle_eval(orc, shape, q)
    want = np.zeros((len(q), 13), np.float32)
    for i in range(len(q)):
        L.orc_kat_bsdf(C.byref(shape), q[i, 0:3].ctypes.data, q[i, 3:6].ctypes.data, q[i, 6:9].ctypes.data, want[i].ctypes.data)
    assert len(q) == 10000
    assert bs.same_bits(got[:, :13], want).all(), bs.describe_mismatch(name, "A+B", q, got[:, :13], want, "array entry vs scalar entry")
    assert np.isin(got[:, 13], (0.0, 1.0)).all()


def _lobe(out):
    """what tells the sampled lobe: delta flag, null flag, eta and the sampled direction (a reflection about the normal, about a microfacet normal, a refraction, the
    cosine-warped sample2 and straight-on are different directions for the same wi and sample2), as bit patterns with one NaN"""
    w = np.ascontiguousarray(out[:, [9, 13, 8, 4, 5, 6]]).copy()
    w[np.isnan(w)] = np.nan
    return w.view(np.uint32)


@pytest.mark.parametrize("name", [m.name for m in bs.catalogue() if m.choice])
def test_family_c_lands_on_the_thresholds_and_the_lobe_changes_there(swept, name):
    m, fam, out, c = swept(name)
    o = out["C"]
    on = c.role == 0
    # the oracle itself reports the threshold it compared with at the re-issued query: it is the target, so the compared value bs.compared_value gives is exact
    reported = o[np.arange(len(o)), 14 + c.level.astype(np.int64)]
    assert bs.same_bits(reported, c.target).all(), (name, "the threshold moved with sample1", int((~bs.same_bits(reported, c.target)).sum()))
    n_exact = int(on.sum())
    print("%s: family C %d queries, %d on a threshold, %d targets without a float32 sample1 (of %d)" % (name, len(o), n_exact, c.missing, len(o) + c.missing))
    assert n_exact >= 1000, (name, n_exact)
    # triples with all three roles present
    key = c.level.astype(np.int64) * (1 << 40) + c.triple
    lobe = _lobe(o)
    below = dict(zip(key[c.role == -1].tolist(), np.nonzero(c.role == -1)[0].tolist()))
    above = dict(zip(key[c.role == 1].tolist(), np.nonzero(c.role == 1)[0].tolist()))
    both = [k for k in below if k in above]
    assert len(both) >= 1000, (name, len(both))
    flips = sum(bool((lobe[below[k]] != lobe[above[k]]).any()) for k in both)
    print("%s: the lobe differs across the threshold in %d of %d triples (%.1f %%)" % (name, flips, len(both), 100.0 * flips / len(both)))
    assert flips >= 0.9 * len(both), (name, flips, len(both))


def _nonzero(x):
    return (x != 0).any(axis=1) if x.ndim == 2 else x != 0


def _kind(m):
    n = m.name
    delta_only = n in ("conductor", "twosided_conductor", "null", "thindielectric") or n.startswith("dielectric")
    transmissive = n in ("null", "thindielectric") or n.startswith("dielectric") or n.startswith("roughdielectric")
    two_sided = n.startswith("twosided")
    mask = n.startswith("mask") or n.startswith("bitmap_opacity")
    return delta_only, transmissive, two_sided, mask


@pytest.mark.parametrize("name", bs.NAMES)
def test_families_meet_the_operand_classes_they_name(swept, name):
    """wi.z > 0, < 0, = +0, = -0, denormal; wo in both hemispheres; and, read from the outputs, both outcomes of the tests on wi.z and wo.z in the chain: a side that
    samples and a side that does not, a wo that has value and density and one that has none"""
    m, fam, out, c = swept(name)
    q = np.concatenate([fam[k] for k in sorted(fam)])
    o = np.concatenate([out[k] for k in sorted(fam)])
    wiz, woz = q[:, 2], q[:, 5]
    bits = wiz.view(np.uint32)
    assert (wiz > 0).any() and (wiz < 0).any() and (bits == 0).any() and (bits == 0x80000000).any()
    assert ((np.abs(wiz) > 0) & (np.abs(wiz) < 2.0 ** -126)).any() and (woz > 0).any() and (woz < 0).any()
    assert (q[:, 6] == 0).any() and (q[:, 6] == bs.ONE_BELOW).any() and (q[:, 7:9] == 0).any() and (q[:, 7:9] == np.float32(bs.S2_MAX)).any()
    if m.textured:
        uv = q[:, 9:11]
        assert (uv < 0).any() and (uv > 1).any() and (uv == 1).any() and (uv.view(np.uint32) == 0x80000000).any() and (np.abs(uv) == 1e6).any()
    if m.framed:
        assert len(np.unique(fam["E"][:, 11:29], axis=0)) == len(bs.frames())
    delta_only, transmissive, two_sided, mask = _kind(m)
    value, pdf, weight = _nonzero(o[:, 0:3]), _nonzero(o[:, 3]), _nonzero(o[:, 10:13])
    nested = o[:, 13] == 0 if mask else np.ones(len(o), bool)      # a mask's null pick has weight 1 on either side: the tests below are about the nested BSDF
    front, back, plane = wiz > 0, wiz < 0, wiz == 0
    assert (weight & front & nested).any(), "no sample from the front"
    if transmissive or two_sided:
        assert (weight & back & nested).any(), "no sample from the back"
    elif not m.framed:          # a one-sided reflector: nothing from behind (under a normal map the perturbed frame may face a grazing wi that the geometry does not)
        assert not (weight & back & nested).any() and not (value & back).any() and not (pdf & back).any()
    if name.startswith("dielectric") or name in ("null", "thindielectric"):
        assert (weight & plane).any()                       # no test on wi.z at all: a direction in the plane is sampled like any other
    elif not m.framed:
        assert not (weight & plane & nested).any(), "a wi in the plane was sampled"
    if delta_only or name == "mask_0":                      # (an opacity of 0 scales every value and density to 0)
        assert not value.any() and not pdf.any()
    else:
        assert (value & pdf & front).any() and (~value & ~pdf & front).any(), "wo with and without value, wi in front"
        if two_sided or name.startswith("roughdielectric"):
            assert (value & pdf & back).any() and (~value & ~pdf & back).any(), "wo with and without value, wi behind"


NAN_CAP = 0.15


@pytest.mark.parametrize("name", bs.NAMES)
def test_nan_rows_stay_a_small_share(swept, name):
    """family A: no NaN and no Inf at all; B - E: NaN rows (a rough lobe under a denormal wi.z, wi and wo both in the plane: DESIGN section 3) in at most 15 % of the rows"""
    m, fam, out, c = swept(name)
    assert np.isfinite(out["A"][:, :14]).all(), (name, int((~np.isfinite(out["A"][:, :14])).any(axis=1).sum()))
    rest = sorted(k for k in fam if k != "A")
    share = {k: float(np.isnan(out[k][:, :14]).any(axis=1).mean()) if len(out[k]) else 0.0 for k in rest}
    rows = sum(len(out[k]) for k in rest)
    total = sum(int(np.isnan(out[k][:, :14]).any(axis=1).sum()) for k in rest) / max(rows, 1)
    print("%s: queries %s; NaN rows %s, B-E together %.2f %%" % (name, {k: len(v) for k, v in fam.items()}, {k: "%.2f %%" % (100 * v) for k, v in share.items()}, 100 * total))
    assert total <= NAN_CAP, (name, share)
