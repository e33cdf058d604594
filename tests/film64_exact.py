#!/usr/bin/env python3
"""The oracle's order-independent image (orc_render_exact: the float32 splat terms summed and developed in float64) of one scene, for tools/time_film64.py, which may
not import the oracle itself (tests/test_loader_and_abi.py: nothing outside tests/ and bench.py's CPU baseline touches it).

    python tests/film64_exact.py scene.xml resx resy spp seed out.npy"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import orc  # noqa: E402


def main(scene, resx, resy, spp, seed, out):
    osc = orc.Scene(scene, dict(resx=int(resx), resy=int(resy)))
    img, _ = osc.render_exact(osc.params(), seed=int(seed), spp=int(spp), threads=os.cpu_count() or 1)
    np.save(out, img)


if __name__ == "__main__":
    main(*sys.argv[1:7])
