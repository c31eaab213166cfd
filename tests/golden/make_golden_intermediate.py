"""Generates tests/golden/intermediate_layers.npz: the token features ChannelVisionTransformer.get_intermediate_layers (models/dichavit.py:665-673)
is meant to return — norm(x) after each of the last n blocks — from the REAL reference (read-only, CPU fp32), for
tests/test_intermediate_layers_gpu.py.  Runs only where the reference is; the GPU tests read the committed fixture.  Reuses make_golden.py's
loader, config, model builder and writer unchanged.

    python tests/golden/make_golden_intermediate.py

The reference's own method raises on every call (it calls prepare_tokens(x, extra_tokens) with the wrong arity), so its intent is computed with
the reference's own modules: fe.prepare_tokens(x, chunk, None, None, {}), then fe.blocks[i] in order, then fe.norm, eval mode; the meta records
that fe.get_intermediate_layers(x) raises TypeError.  The cases are the attention fixture's (make_golden_attn.py), with oracle.make_state's
weights as they are (no sharpening), one image each.  The tokens are stored in float16 to keep the file small (relative rounding 2^-11: far
inside the tests' 3e-2 bound).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from oracle import dichavit_oracle as orc  # noqa: E402

# (name, cfg overrides, mapper, chunk, n_channels, model img, input img, num_classes, B, state seed, batch seed, n)
CASES = [
    ("small", dict(patch_size=8), {"train": [0, 1, 2, 3, 4]}, "train", 5, 32, 32, 6, 1, 201, 202, 4),
    ("sub", dict(patch_size=8), {"train": [0, 1, 2, 3, 4], "sub": [0, 2, 4]}, "sub", 5, 32, 32, 6, 1, 211, 212, 1),
    ("tiny48", dict(pretrained_model_name="tiny", patch_size=8), {"train": [0, 1, 2]}, "train", 3, 32, 48, 5, 1, 221, 222, 2),
    ("base", dict(pretrained_model_name="base", patch_size=8), {"train": [0, 1, 2]}, "train", 3, 32, 32, 5, 1, 231, 232, 1),
]


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
    torch.manual_seed(0)
    dichavit, _ = mg.load_reference()
    arrays, cases = {}, []
    for name, kw, mapper, chunk, n_ch, img, img_in, K, B, seed, bseed, n in CASES:
        cfg = mg.base_cfg(**kw)
        model, _ = mg.build(dichavit, cfg, mapper, n_ch, img, K, seed)
        model.eval()
        fe = model.feature_extractor
        x, _ = orc.make_batch(bseed, B, len(mapper[chunk]), img_in, K)
        depth = len(fe.blocks)
        blocks = list(range(depth - n, depth))
        try:
            fe.get_intermediate_layers(x)
            raises = None
        except Exception as e:  # noqa: BLE001 — the kind of failure is what gets recorded
            raises = type(e).__name__
        with torch.no_grad():
            t, _ = fe.prepare_tokens(x, chunk, None, None, {})
            for i, blk in enumerate(fe.blocks):
                t = blk(t)
                if i in blocks:
                    o = fe.norm(t)
                    arrays[f"{name}/block{i}"] = o.numpy().astype(np.float16)
                    print(f"  {name} block {i}: {tuple(o.shape)}, max |.| {float(o.abs().max()):.3f}")
        cases.append(dict(name=name, cfg=cfg, mapper=mapper, chunk=chunk, n_channels=n_ch, img=img, img_in=img_in, num_classes=K, B=B, seed=seed,
                          batch_seed=bseed, n=n, blocks=blocks, reference_method_raises=raises))
    assert all(c["reference_method_raises"] == "TypeError" for c in cases), [c["reference_method_raises"] for c in cases]
    mg.save("intermediate_layers", dict(cases=cases), arrays)


if __name__ == "__main__":
    main()
