"""Generates tests/golden/attn_maps.npz: attention maps of ChannelVisionTransformer.get_last_selfattention (models/dichavit.py:654-663) from
the REAL reference (read-only, CPU fp32), for tests/test_attn_maps_gpu.py.  Runs only where the reference is; the GPU tests read the committed
fixture.  Reuses make_golden.py's loader, config, model builder and writer unchanged.

    python tests/golden/make_golden_attn.py

Sharpened maps: with oracle.make_state's weights the maps are almost uniform (row max ~0.017 against 1/81), so a test against them barely tells
a right kernel from a wrong one.  The q and k rows ([:2D]) of every blocks.i.attn.qkv.weight are multiplied by QK_MULT after loading the state
(row maxima up to ~0.95); the tests apply the same multiplier.  DiChaViT-B takes BASE_QK_MULT instead: its 768-wide q . k at x4 saturates the
softmax (row maxima 1.000), where the bf16 rounding of the qkv output alone moves the map by 0.09 of its maximum (a CPU emulation of that rounding
on the reference: mean total variation 0.026 at x4, against <= 0.006 for the other cases).  Every case runs in eval mode on one image.  The
fixture holds the maps and a JSON meta only; the maps are stored in float16 to keep the file small (relative rounding 2^-11, a total variation of
at most 2.5e-4 per row: far inside the tests' bounds).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from oracle import dichavit_oracle as orc  # noqa: E402

QK_MULT = 4.0
BASE_QK_MULT = 2.0

# (name, cfg overrides, mapper, chunk, n_channels, model img, input img, num_classes, B, state seed, batch seed, layers)
CASES = [
    ("small", dict(patch_size=8), {"train": [0, 1, 2, 3, 4]}, "train", 5, 32, 32, 6, 1, 201, 202, [0, 5, 11]),
    ("sub", dict(patch_size=8), {"train": [0, 1, 2, 3, 4], "sub": [0, 2, 4]}, "sub", 5, 32, 32, 6, 1, 211, 212, [3]),
    ("tiny48", dict(pretrained_model_name="tiny", patch_size=8), {"train": [0, 1, 2]}, "train", 3, 32, 48, 5, 1, 221, 222, [11]),
    ("base", dict(pretrained_model_name="base", patch_size=8), {"train": [0, 1, 2]}, "train", 3, 32, 32, 5, 1, 231, 232, [11]),
]


def sharpen(model, mult):
    D = model.feature_extractor.embed_dim
    with torch.no_grad():
        for blk in model.feature_extractor.blocks:
            blk.attn.qkv.weight[:2 * D] *= mult


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
    torch.manual_seed(0)
    dichavit, _ = mg.load_reference()
    arrays, cases = {}, []
    for name, kw, mapper, chunk, n_ch, img, img_in, K, B, seed, bseed, layers in CASES:
        cfg = mg.base_cfg(**kw)
        model, _ = mg.build(dichavit, cfg, mapper, n_ch, img, K, seed)
        mult = BASE_QK_MULT if kw.get("pretrained_model_name") == "base" else QK_MULT
        sharpen(model, mult)
        model.eval()
        fe = model.feature_extractor
        x, _ = orc.make_batch(bseed, B, len(mapper[chunk]), img_in, K)
        case = dict(name=name, cfg=cfg, mapper=mapper, chunk=chunk, n_channels=n_ch, img=img, img_in=img_in, num_classes=K, B=B, seed=seed,
                    batch_seed=bseed, layers=layers, qk_mult=mult)
        with torch.no_grad():
            for li in layers:
                a = fe.get_last_selfattention(x, chunk=chunk, layer_idx=li)
                arrays[f"{name}/layer{li}"] = a.numpy().astype(np.float16)
                rs = a.sum(-1)
                print(f"  {name} layer {li}: {tuple(a.shape)}, row-sum err {float((rs - 1).abs().max()):.2e}, row max {float(a.max()):.3f}")
            if name == "small":
                # the reference's own answers for the default and an out-of-range index: its loop tests i == layer_idx, so both give None
                case["none_for"] = [li for li in (-1, 12) if fe.get_last_selfattention(x, chunk=chunk, layer_idx=li) is None]
        cases.append(case)
    mg.save("attn_maps", dict(qk_mult=QK_MULT, cases=cases), arrays)


if __name__ == "__main__":
    main()
