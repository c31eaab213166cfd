"""Generates tests/golden/tps_warp.npz: outputs of the REAL reference's thin-plate-spline warp (datasets/tps_transform.py: tps_warp_2, which the
train transform's TPSTransform reaches through tps_transform) for fixed control points, for tests/test_device_augment_{cpu,gpu}.py.  Runs only
where the reference is; the tests read the committed fixture.  torchvision and matplotlib, which the reference module imports and the warp never
calls, are stubbed in sys.modules when they are not installed.

Images are random integers 0..255, stored as uint8 and handed to the reference as float32 (map_coordinates answers in the input's dtype: a
uint8 image would come back rounded); src is the reference's 3 x 3 regular grid on [0, W], dst = src + a uniform displacement of +-scale W:
    w31 (3 coarse points, steps - 1 = 2 exactly), w64, w160 (CHAMMI CP's size), w224 with one channel, scale 0.1 (the recipe's);
    zero: dst = src — NOT the identity (the coarse grid is upsampled with steps - 1 where it has int(steps) - 1 intervals);
    far: scale 0.45, with the seed (of 400 tried) whose coordinates reach furthest: -44 .. 148.9 at W = 64, past 2 W, where the reflect fold
    has turned twice.

    python tests/golden/make_golden_tps.py
"""
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

CASES = [dict(name="w31", W=31, C=3, scale=0.1), dict(name="w64", W=64, C=5, scale=0.1), dict(name="w160", W=160, C=3, scale=0.1),
         dict(name="w224", W=224, C=1, scale=0.1), dict(name="zero", W=64, C=1, scale=0.0), dict(name="far", W=64, C=3, scale=0.45, seed=2074)]


def load_tps():
    for name in ("torchvision", "torchvision.transforms", "torchvision.datasets", "matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
            parent, _, leaf = name.rpartition(".")
            if parent:
                setattr(sys.modules[parent], leaf, m)
    sys.modules["torchvision.transforms"].transforms = sys.modules["torchvision.transforms"]
    sys.path.insert(0, os.path.join(REF, "datasets"))
    return importlib.import_module("tps_transform")


def main():
    tps = load_tps()
    out, meta = {}, []
    for k, case in enumerate(CASES):
        rng = np.random.default_rng(case.get("seed", 1000 + k))
        W, C = case["W"], case["C"]
        img = rng.integers(0, 256, size=(C, W, W), dtype=np.uint8)
        hwc = np.moveaxis(img, 0, 2).astype(np.float32)
        src = tps._get_regular_grid(hwc, points_per_dim=3)
        dst = src + rng.uniform(-case["scale"] * W, case["scale"] * W, src.shape)
        res = tps.tps_warp_2(hwc, dst, src)
        assert res.dtype == np.float32 and res.shape == hwc.shape
        n = case["name"]
        out[n + "_img"], out[n + "_src"], out[n + "_dst"], out[n + "_out"] = img, src, dst, np.ascontiguousarray(np.moveaxis(res, 2, 0))
        meta.append(case)
    path = os.path.join(HERE, "tps_warp.npz")
    np.savez(path, meta=np.array(json.dumps(dict(cases=meta))), **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
