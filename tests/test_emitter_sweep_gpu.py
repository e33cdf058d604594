"""The device emitter chain against the oracle on dense and boundary inputs: every scene of tests/emitter_sweep.py through every (AREA, MESH, SPEC) level of the shade
kernels the render path can run on it (dtof_emitter_eval: sample_emitter_direction, emitter_pdf_direction and the environment's density and value, the functions
k_shade calls), against orc_kat_emitter_n on the same queries.  The rule is the project's own contract: all output words equal as bit patterns (two NaNs equal
whatever their payload), no tolerance, and no word is masked.  test_emitter_sweep_cpu.py shows, on the oracle alone, that these inputs sit on and around every
compare of the chain; profiles/emitter_sweep_mutations.txt records what the module catches."""
import time

import numpy as np
import pytest

import emitter_sweep as es

pytestmark = pytest.mark.gpu
DTOF_ERR_INVALID = 1
F32 = np.float32
CASES = [(x.name, lv) for x in es.catalogue() for lv in x.levels]


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    return es.write_fixtures(tmp_path_factory.mktemp("emitter_sweep"))


@pytest.fixture(scope="module")
def swept(mi, orc, fixtures):
    """name -> (entry, device scene, {(mode, family, shape): queries}, {...: oracle outputs}, {level: {...: device outputs as uint32}}); the last entry is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            e = {x.name: x for x in es.catalogue(fixtures)}[name]
            osc = orc.Scene(e.xml, {}, is_string=True)
            t0 = time.time()
            fam, _ = es.families(e, orc, osc)
            want = {k: es.oracle_eval(orc, osc, k[0], q, k[2])[:, :es.N_OUT[k[0]]] for k, q in fam.items()}
            print("%s: %s queries, oracle %.2f s" % (name, {k: len(q) for k, q in fam.items()}, time.time() - t0))
            cache[name] = (e, mi.load_string(e.xml), fam, want, {}, osc)
        return cache[name][:5]
    return get


def _device(mi, entry, level):
    e, scene, fam, want, got = entry
    if level not in got:
        got[level] = {}
        for k, q in fam.items():
            rc, out = es.device_eval(mi, scene, k[0], level, q, k[2])
            assert rc == 0, (e.name, level, k, mi._lib().dtof_last_error())
            assert not (out == es.CANARY).any(), "%s, level %d, %s: %d output words were never written" % (e.name, level, k, int((out == es.CANARY).sum()))
            got[level][k] = out
    return got[level]


@pytest.mark.parametrize("name,level", CASES)
def test_device_emitter_chain_equals_the_oracle(mi, swept, name, level):
    entry = swept(name)
    e, scene, fam, want, _ = entry
    got = _device(mi, entry, level)
    what = "%s, level %d %s" % (name, level, es.LEVEL_NAMES[level])
    wrong = [es.describe_mismatch(what, k[0], "%s (mode %d, shape %d)" % (k[1], k[0], k[2]), fam[k], got[k], want[k]) for k in sorted(fam) if not es.same_bits(got[k], want[k]).all()]
    assert not wrong, "\n".join(wrong)
    # the levels that can run on this scene agree with each other
    for other in e.levels:
        if other < level:
            prev = _device(mi, entry, other)
            wrong += [es.describe_mismatch(what, k[0], k[1], fam[k], got[k], prev[k], "against level %d" % other) for k in sorted(fam) if not es.same_bits(got[k], prev[k]).all()]
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("name", es.NAMES)
def test_level_minus_one_is_what_a_render_runs(mi, swept, name):
    """level = -1 is accepted for every scene and equals the level scene_traits() implies, in every mode the scene has; Scene.emitter_eval is the same call"""
    entry = swept(name)
    e, scene, fam, want, _ = entry
    explicit = _device(mi, entry, e.traits_level)
    for k, q in fam.items():
        rc, auto = es.device_eval(mi, scene, k[0], -1, q, k[2])
        assert rc == 0, mi._lib().dtof_last_error()
        assert np.array_equal(auto, explicit[k]), es.describe_mismatch(name, k[0], k[1], q, auto, explicit[k], "level = -1 against level %d" % e.traits_level)
        assert np.array_equal(scene.emitter_eval(k[0], q[:1000], shape_index=k[2]).view(np.uint32), auto[:1000])


def _refused(mi, scene, mode, level, q, shape=-1):
    rc, out = es.device_eval(mi, scene, mode, level, q, shape)
    return rc == DTOF_ERR_INVALID and bool((out == es.CANARY).all())


@pytest.mark.parametrize("name", es.NAMES)
def test_refusals_write_nothing(mi, swept, name):
    """a level the render path could never run on the scene, a level that is none, a shape without an emitter or out of range, a missing environment, a float that is
    not finite, a draw outside [0, 1): DTOF_ERR_INVALID, the output buffer untouched"""
    e, scene, fam, want, _ = swept(name)
    a = fam[(0, "A", -1)][:256]
    for level in [lv for lv in es.ALL_LEVELS if lv not in e.levels] + [-2, 7]:
        assert _refused(mi, scene, 0, level, a), (name, level)
    ok = e.levels[-1]
    assert es.device_eval(mi, scene, 0, ok, a)[0] == 0
    n_shapes = len(e.hit_shapes) + 1                                  # the floor comes last and carries no emitter
    d = np.zeros((4, 11), F32); d[:, 3:6] = 1; d[:, 8] = 1
    for shape in (n_shapes - 1, n_shapes, -1, 10 ** 6):
        assert _refused(mi, scene, 1, ok, d, shape), (name, shape)
    for shape in e.hit_shapes:
        assert es.device_eval(mi, scene, 1, ok, d, shape)[0] == 0
        for lv in (0, 2, 6):                                          # (ineligible for a scene with an area light; the entry's own `!area` guard behind that rule cannot be reached)
            assert _refused(mi, scene, 1, lv, d, shape)
    if not e.hit_shapes:                                              # an eligible level WITHOUT AREA and with it: the floor carries no emitter either way
        for lv in e.levels:
            assert _refused(mi, scene, 1, lv, d, 0), (name, lv)
    dirs = np.array([[0, 0, 1], [1, 0, 0]], F32)
    assert (es.device_eval(mi, scene, 2, ok, dirs)[0] == 0) if e.env else _refused(mi, scene, 2, ok, dirs), name
    # the validation rule of the queries
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(5):
            q = a.copy(); q[17, col] = bad
            assert _refused(mi, scene, 0, ok, q), (name, bad, col)
    for bad in (1.0, np.nextafter(F32(1), F32(2)), -2.0 ** -149, -0.5, 2.0, 3.0e38):
        for col in (3, 4):
            q = a.copy(); q[255, col] = bad
            assert _refused(mi, scene, 0, ok, q), (name, bad, col)
    for shape in e.hit_shapes:
        q = np.tile(d, (8, 1)); q[13, 9] = np.nan
        assert _refused(mi, scene, 1, ok, q, shape)
        q = np.tile(d, (8, 1)); q[31, 2] = np.inf
        assert _refused(mi, scene, 1, ok, q, shape)
    if e.env:
        q = np.tile(dirs, (8, 1)); q[5, 1] = np.nan
        assert _refused(mi, scene, 2, ok, q)


def test_a_scene_without_emitters_is_refused(mi):
    scene = mi.load_string('<scene version="3.0.0">%s</scene>' % es.FLOOR)
    q = np.zeros((4, 5), F32)
    for level in (-1, 0, 3, 5):
        assert _refused(mi, scene, 0, level, q), level
