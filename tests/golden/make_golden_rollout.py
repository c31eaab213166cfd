"""Generates tests/golden/attn_rollout.npz: attention rollout of the REAL reference's own maps (read-only, CPU fp32), for
tests/test_attention_rollout_{cpu,gpu}.py.  Runs only where the reference is; the tests read the committed fixture.  Reuses make_golden.py's
loader, config, model builder and writer and make_golden_attn.py's cases and sharpening unchanged, except that every case runs on B = 2 images.

    python tests/golden/make_golden_rollout.py

For each case all twelve maps come from the reference's get_last_selfattention(x, chunk=..., layer_idx=i) in eval mode and are rolled in
float64 (tests/attention_rollout_ref.py: mean head fusion, residual 0.5, one-hot CLS start, last block first).  The fixture stores
rollout[s] for EVERY start_layer s = 0 .. 11 as float32 [12, B, N], and a JSON meta.  Every start layer on purpose: the full rollout (s = 0) of
these models lies close to the uniform vector, and dropping a block from it moves it by very little, so a comparison at s = 0 alone cannot tell a
right implementation from several wrong ones; the same wrong variants stand out at high s (at s = 11 the answer is 0.5 e_0 + 0.5 times the
head-mean CLS row).  The generator prints those distances."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_attn as mga  # noqa: E402
from attention_rollout_ref import rollout, tv  # noqa: E402
from oracle import dichavit_oracle as orc  # noqa: E402

B = 2
RESIDUAL = 0.5


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
    torch.manual_seed(0)
    dichavit, _ = mg.load_reference()
    arrays, cases = {}, []
    for name, kw, mapper, chunk, n_ch, img, img_in, K, _, seed, bseed, _ in mga.CASES:
        cfg = mg.base_cfg(**kw)
        model, _ = mg.build(dichavit, cfg, mapper, n_ch, img, K, seed)
        mult = mga.BASE_QK_MULT if kw.get("pretrained_model_name") == "base" else mga.QK_MULT
        mga.sharpen(model, mult)
        model.eval()
        fe = model.feature_extractor
        depth = len(fe.blocks)
        x, _ = orc.make_batch(bseed, B, len(mapper[chunk]), img_in, K)
        with torch.no_grad():
            maps = [fe.get_last_selfattention(x, chunk=chunk, layer_idx=i) for i in range(depth)]
        rolls = torch.stack([rollout(maps, s, RESIDUAL) for s in range(depth)])  # [depth, B, N] float64
        N = rolls.shape[-1]
        arrays[f"{name}/rollout"] = rolls.numpy().astype(np.float32)
        cases.append(dict(name=name, cfg=cfg, mapper=mapper, chunk=chunk, n_channels=n_ch, img=img, img_in=img_in, num_classes=K, B=B, seed=seed,
                          batch_seed=bseed, qk_mult=mult, depth=depth, N=N, residual=RESIDUAL))
        uniform = torch.full((B, N), 1.0 / N, dtype=torch.float64)
        ascending = torch.zeros(B, N, dtype=torch.float64)
        ascending[:, 0] = 1.0
        for A in maps:  # the wrong order: block 0 applied first
            ascending = RESIDUAL * ascending + (1 - RESIDUAL) * torch.einsum("bq,bqk->bk", ascending, A.double().mean(1))
        print(f"  {name}: N {N}; row-sum err {float((rolls.sum(-1) - 1).abs().max()):.2e}; TV(s=0, uniform) {tv(rolls[0], uniform):.3e}; "
              f"TV(s=0, without block 11) {tv(rolls[0], rollout(maps[:-1], 0, RESIDUAL)):.3e}; TV(s=0, ascending order) {tv(rolls[0], ascending):.3e}; "
              f"TV(s=11, s=0) {tv(rolls[11], rolls[0]):.3e}; min rollout[11][:, 0] {float(rolls[11][:, 0].min()):.4f}")
    mg.save("attn_rollout", dict(cases=cases), arrays)


if __name__ == "__main__":
    main()
