"""The device BSDF chain against the oracle on dense and boundary inputs: every material of tests/bsdf_sweep.py through every instantiation of
`bsdf_eval_pdf_sample<SPEC>` the render path can run on it (dtof_bsdf_eval_ex), against orc_kat_bsdf_n on the same queries.  The rule is the project's own contract:
all 14 output words equal as bit patterns (two NaNs equal whatever their payload), no tolerance.  test_bsdf_sweep_cpu.py shows, on the oracle alone, that these
inputs reach the thresholds of the lobe choices and the operand classes they name; profiles/bsdf_sweep_mutations.txt records what the module catches."""
import time

import numpy as np
import pytest

import bsdf_sweep as bs

pytestmark = pytest.mark.gpu
DTOF_ERR_INVALID = 1
CASES = [(m.name, spec) for m in bs.catalogue() for spec in m.specs]
TRAITS_SPEC = {m.name: 0 if m.specs[0] == 0 else 2 if m.specs == (2,) else 1 for m in bs.catalogue()}   # what scene_traits() picks for the one-shape scene


@pytest.fixture(scope="module")
def texdir(tmp_path_factory):
    return bs.write_textures(tmp_path_factory.mktemp("bsdf_sweep"))


@pytest.fixture(scope="module")
def swept(mi, orc, texdir):
    """name -> (material, device scene, {family: queries}, {family: oracle outputs}, {spec: {family: device outputs as uint32}}); the last material is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            m = {x.name: x for x in bs.catalogue(texdir)}[name]
            xml = bs.SCENE % m.bsdf
            osc = orc.Scene(xml, {}, is_string=True)
            t0 = time.time()
            fam, _ = bs.families(m, lambda q: bs.oracle_eval(orc, osc.c.shapes[0], q))
            want = {k: bs.oracle_eval(orc, osc.c.shapes[0], q)[:, :14] for k, q in fam.items()}
            print("%s: %s queries, oracle %.2f s" % (name, {k: len(q) for k, q in fam.items()}, time.time() - t0))
            cache[name] = (m, mi.load_string(xml), fam, want, {}, osc)
        return cache[name][:5]
    return get


def _device(mi, entry, spec):
    m, scene, fam, want, got = entry
    if spec not in got:
        got[spec] = {}
        for k, q in fam.items():
            rc, out = bs.device_eval(mi, scene, spec, q)
            assert rc == 0, (m.name, spec, k, mi._lib().dtof_last_error())
            assert not (out == bs.CANARY).any(), "%s, SPEC %d, family %s: %d output words were never written" % (m.name, spec, k, int((out == bs.CANARY).sum()))
            got[spec][k] = out
    return got[spec]


@pytest.mark.parametrize("name,spec", CASES)
def test_device_chain_equals_the_oracle(mi, swept, name, spec):
    entry = swept(name)
    m, scene, fam, want, _ = entry
    got = _device(mi, entry, spec)
    wrong = [bs.describe_mismatch("%s, SPEC %d" % (name, spec), k, fam[k], got[k], want[k]) for k in sorted(fam) if not bs.same_bits(got[k], want[k]).all()]
    assert not wrong, "\n".join(wrong)
    # the instantiations that can run on this shape agree with each other
    for other in m.specs:
        if other < spec:
            prev = _device(mi, entry, other)
            wrong += [bs.describe_mismatch("%s, SPEC %d" % (name, spec), k, fam[k], got[k], prev[k], "against SPEC %d" % other) for k in sorted(fam)
                      if not bs.same_bits(got[k], prev[k]).all()]
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("name", bs.NAMES)
def test_spec_minus_one_is_what_a_render_runs_and_the_old_entry_is_the_flat_frame(mi, swept, name):
    """spec = -1 is accepted for every material (so it names an eligible instantiation) and equals the SPEC scene_traits() implies; dtof_bsdf_eval, the 11-float entry of
    the reference's unit tests, is dtof_bsdf_eval_ex with the identity frame and spec = 2, on all of family A"""
    entry = swept(name)
    m, scene, fam, want, _ = entry
    a = fam["A"]
    rc, auto = bs.device_eval(mi, scene, -1, a)
    assert rc == 0, mi._lib().dtof_last_error()
    explicit = _device(mi, entry, TRAITS_SPEC[name])["A"]
    assert np.array_equal(auto, explicit), bs.describe_mismatch(name, "A", a, auto, explicit, "spec = -1 against SPEC %d" % TRAITS_SPEC[name])
    assert (a[:, 11:29] == bs.FLAT).all()
    q11 = np.ascontiguousarray(a[:, :11])
    old = np.full((len(a), 14), bs.CANARY, np.uint32)
    assert mi._lib().dtof_bsdf_eval(scene._h, 0, len(q11), q11.ctypes.data, old.ctypes.data) == 0
    new = _device(mi, entry, 2)["A"]
    assert np.array_equal(old, new), bs.describe_mismatch(name, "A", a, old, new, "dtof_bsdf_eval against dtof_bsdf_eval_ex(spec = 2)")
    assert np.array_equal(scene.bsdf_eval(0, q11[:1000], spec=2).view(np.uint32), new[:1000])
    assert np.array_equal(scene.bsdf_eval(0, a[:1000]).view(np.uint32), auto[:1000])              # 29-float rows, spec = -1


@pytest.mark.parametrize("name", bs.NAMES)
def test_ineligible_instantiations_are_refused_and_write_nothing(mi, swept, name):
    """SPEC 0 on anything but an untextured (twosided) diffuse, SPEC 1 on a blendbsdf or a two-BSDF twosided, and a spec that is no instantiation: DTOF_ERR_INVALID,
    the output buffer untouched"""
    m, scene, fam, want, _ = swept(name)
    q = fam["B"][:256]
    for spec in [s for s in (0, 1, 2) if s not in m.specs] + [-2, 3]:
        rc, out = bs.device_eval(mi, scene, spec, q)
        assert rc == DTOF_ERR_INVALID, (name, spec, rc)
        assert (out == bs.CANARY).all(), (name, spec, "a refused call wrote to its output")
    for spec in m.specs:
        assert bs.device_eval(mi, scene, spec, q)[0] == 0, (name, spec)
    rc, out = bs.device_eval(mi, scene, 2, q, shape_index=10 ** 6)
    assert rc == DTOF_ERR_INVALID and (out == bs.CANARY).all()
