"""Generates tests/golden/attn_relevance.npz: gradient-weighted attention relevance (Chefer, Gur & Wolf 2021) of the REAL reference's own
attention maps and their gradients (read-only, CPU float64), for tests/test_attention_relevance_{cpu,gpu}.py.  Runs only where the reference is;
the tests read the committed fixture.  Reuses make_golden.py's loader, config, model builder and writer and make_golden_attn.py's cases and
sharpening unchanged, except that every case runs on B = 2 images.

    python tests/golden/make_golden_relevance.py

For each case the reference model runs in eval mode and in double.  A forward hook on every blk.attn keeps the `attn` its forward returns
(models/vit.py:121-144) and asks autograd to retain its gradient; logits.gather(1, target).sum().backward() fills them, and
tests/attention_relevance_ref.py turns maps and gradients into the relevance (mean head fusion, relu, one-hot CLS start, last block first).
Two targets per image — the reference's top and bottom class, RECORDED in the meta so that no argmax can flip on the GPU — and EVERY
start_layer: relevance float32 [2, depth, B, N].

The same forward is run again with every nn.Linear's input, weight and output rounded to bf16 (straight-through: the backward is left in
float64), the arithmetic the HIP path's forward has.  The meta stores, per case, the largest distance of that emulation from float64 over targets
and start layers: `emu_tv`, the total variation of the normalised patch relevance r[:, 1:] / sum, and `emu_cls_rel` / `emu_sum_rel`, the
relative errors of r[:, 0] and of sum r[:, 1:].  The GPU tests hold the model to three times these.  Printed per case: the distances from the
right answer to the wrong ones (the other target, no relu, ascending block order, plain rollout)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_attn as mga  # noqa: E402
from attention_relevance_ref import normalised_patches, relevance, tv  # noqa: E402
from attention_rollout_ref import rollout  # noqa: E402
from oracle import dichavit_oracle as orc  # noqa: E402

B = 2


def maps_and_grads(model, x, chunk, target):
    """One forward and one backward of sum_b logits[b, target[b]]: (logits, the twelve maps, their gradients), float64."""
    kept = []

    def keep(module, inputs, output):  # returns None: a hook that returns a value would replace the module's output
        output[1].retain_grad()
        kept.append(output[1])

    handles = [blk.attn.register_forward_hook(keep) for blk in model.feature_extractor.blocks]
    try:
        model.zero_grad(set_to_none=True)
        logits = model(x, chunk, None, init_first_layer=None, new_channel_init=None)
        if target is not None:
            logits.gather(1, target.view(-1, 1)).sum().backward()
    finally:
        for h in handles:
            h.remove()
    return logits.detach(), [a.detach() for a in kept], [a.grad for a in kept]


class bf16_linears:
    """Every nn.Linear computes bf16(bf16(x) bf16(W)^T + b) while active; the rounding is straight-through for the backward."""

    @staticmethod
    def _round(t):
        return t + (t.to(torch.bfloat16).to(t.dtype) - t).detach()

    def __enter__(self):
        self.real = torch.nn.functional.linear
        torch.nn.functional.linear = lambda x, w, b=None: self._round(self.real(self._round(x), self._round(w), b))

    def __exit__(self, *exc):
        torch.nn.functional.linear = self.real


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
        model.eval().double()
        depth = len(model.feature_extractor.blocks)
        x, _ = orc.make_batch(bseed, B, len(mapper[chunk]), img_in, K)
        x = x.double()
        with torch.no_grad():
            logits = model(x, chunk, None, init_first_layer=None, new_channel_init=None)
        targets = torch.stack([logits.argmax(1), logits.argmin(1)])  # [2, B]: top and bottom class
        rel = torch.empty(2, depth, B, 0, dtype=torch.float64)
        emu_tv = emu_cls = emu_sum = 0.0
        wrong = dict(no_relu=0.0, ascending=0.0, rollout=0.0)
        for ti in range(2):
            _, maps, grads = maps_and_grads(model, x, chunk, targets[ti])
            with bf16_linears():
                _, emaps, egrads = maps_and_grads(model, x, chunk, targets[ti])
            if rel.shape[-1] == 0:
                rel = torch.empty(2, depth, B, maps[0].shape[-1], dtype=torch.float64)
            for s in range(depth):
                r = relevance(maps, grads, s)
                e = relevance(emaps, egrads, s)
                rel[ti, s] = r
                emu_tv = max(emu_tv, tv(normalised_patches(e), normalised_patches(r)))
                emu_cls = max(emu_cls, float(((e[:, 0] - r[:, 0]).abs() / r[:, 0]).max()))
                emu_sum = max(emu_sum, float(((e[:, 1:].sum(-1) - r[:, 1:].sum(-1)).abs() / r[:, 1:].sum(-1)).max()))
            # the wrong answers, at start_layer 0
            r0 = normalised_patches(rel[ti, 0])
            raw = torch.zeros(B, maps[0].shape[-1], dtype=torch.float64)
            asc = raw.clone()
            raw[:, 0] = asc[:, 0] = 1.0
            for l in range(depth - 1, -1, -1):
                raw = raw + torch.einsum("bq,bqk->bk", raw, (grads[l] * maps[l]).mean(1))
            for l in range(depth):
                asc = asc + torch.einsum("bq,bqk->bk", asc, (grads[l] * maps[l]).clamp(min=0).mean(1))
            wrong["no_relu"] = max(wrong["no_relu"], tv(raw[:, 1:] / raw[:, 1:].sum(-1, keepdim=True), r0))
            wrong["ascending"] = max(wrong["ascending"], tv(normalised_patches(asc), r0))
            wrong["rollout"] = max(wrong["rollout"], tv(normalised_patches(rollout(maps, 0, 0.5)), r0))
        N = rel.shape[-1]
        other = [tv(normalised_patches(rel[0, s]), normalised_patches(rel[1, s])) for s in range(depth)]
        arrays[f"{name}/relevance"] = rel.numpy().astype(np.float32)
        cases.append(dict(name=name, cfg=cfg, mapper=mapper, chunk=chunk, n_channels=n_ch, img=img, img_in=img_in, num_classes=K, B=B, seed=seed,
                          batch_seed=bseed, qk_mult=mult, depth=depth, N=N, targets=targets.tolist(), emu_tv=emu_tv, emu_cls_rel=emu_cls,
                          emu_sum_rel=emu_sum))
        print(f"  {name}: N {N}; targets {targets.tolist()}; emulation: tv {emu_tv:.2e}, r[:,0] rel {emu_cls:.2e}, sum r[:,1:] rel {emu_sum:.2e}; "
              f"sum r[:,1:] at s=0 {rel[:, 0, :, 1:].sum(-1).min():.3f} .. {rel[:, 0, :, 1:].sum(-1).max():.3f}, at s={depth - 1} "
              f"{rel[:, -1, :, 1:].sum(-1).min():.4f} .. {rel[:, -1, :, 1:].sum(-1).max():.4f}; TV to the other target over s "
              f"{min(other):.3f} .. {max(other):.3f}; at s=0 TV to no relu {wrong['no_relu']:.3f}, ascending order {wrong['ascending']:.3f}, "
              f"plain rollout {wrong['rollout']:.3f}")
    mg.save("attn_relevance", dict(cases=cases), arrays)


if __name__ == "__main__":
    main()
