"""Generates tests/golden/input_grad.npz: the gradient of a loss with respect to the INPUT IMAGES (x.grad) from the REAL reference (read-only,
CPU fp32), for tests/test_input_grad_cpu.py and tests/test_input_grad_gpu.py.  Runs only where the reference is; the tests read the committed
fixture.  Reuses make_golden.py's loader, config, model builder and writer unchanged.

    python tests/golden/make_golden_input_grad.py

Cases:
  so2sat  train mode, P 8, 32 x 32, 5 channels, B 2, ortho and proxy terms on; loss = CE + extra
  sub     eval, chunk "sub" of a non-identity mapper with training_chunks and new_channel_init "avg_2"; sum_b logits[b, y_b]
  jumpcp  eval, JUMP-CP-S: 8 channels, 224 x 224, P 16, B 1; logits[0, y_0]
  ragged  eval, a 36 x 44 image (P 8: neither side a multiple of P, H != W); sum_b logits[b, y_b]
  base    eval, DiChaViT-B (D 768), P 8, 32 x 32, 3 channels; sum_b logits[b, y_b]
Images come from oracle.make_batch(batch seed, B, C, max(H, W), K), cropped to [:H, :W].  Gradients are stored in float16 after division by a
per-case power-of-two scale (`<case>/scale`; dx = grad * scale): the raw values are around 1e-6 .. 1e-3 and would underflow float16.  The jumpcp
case keeps its top 112 image rows only (all 8 channels) to keep the file small.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from oracle import dichavit_oracle as orc  # noqa: E402

# (name, cfg overrides, mapper, chunk, training_chunks, new_channel_init, n_channels, model img, (H, W), num classes, B, train, seeds, rows kept)
CASES = [
    ("so2sat", dict(patch_size=8, ortho_loss_v1_lambda=0.1, gamma_s=0.5, proxy_loss_lambda=0.01), {"train": [0, 1, 2, 3, 4]}, "train", None, None,
     5, 32, (32, 32), 17, 2, True, (301, 302), None),
    ("sub", dict(patch_size=8), {"train": [0, 1, 2, 3, 4], "sub": [0, 5, 3]}, "sub", "train", "avg_2", 7, 32, (32, 32), 9, 2, False,
     (311, 312), None),
    ("jumpcp", dict(), {"train": list(range(8))}, "train", None, None, 8, 224, (224, 224), 161, 1, False, (321, 322), 112),
    ("ragged", dict(patch_size=8), {"train": [0, 1, 2, 3]}, "train", None, None, 4, 32, (36, 44), 6, 2, False, (331, 332), None),
    ("base", dict(pretrained_model_name="base", patch_size=8), {"train": [0, 1, 2]}, "train", None, None, 3, 32, (32, 32), 5, 2, False,
     (341, 342), None),
]


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
    torch.manual_seed(0)
    dichavit, _ = mg.load_reference()
    arrays, cases = {}, []
    for name, kw, mapper, chunk, tchunks, init, n_ch, img, (H, W), K, B, train, (seed, bseed), rows in CASES:
        cfg = mg.base_cfg(**kw)
        model, _ = mg.build(dichavit, cfg, mapper, n_ch, img, K, seed)
        model.train(train)
        x, y = orc.make_batch(bseed, B, len(mapper[chunk]), max(H, W), K)
        x = x[:, :, :H, :W].contiguous().requires_grad_(True)
        if train:
            out, extra = model(x, chunk, None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            loss = torch.nn.CrossEntropyLoss()(out, y) + extra
        else:
            out = model(x, chunk, tchunks, init_first_layer=None, new_channel_init=init)
            loss = out.gather(1, y[:, None]).sum()
        loss.backward()
        g = x.grad.detach().double().numpy()
        if rows is not None:
            g = g[:, :, :rows]
        scale = float(2.0 ** np.ceil(np.log2(np.abs(g).max() / 60000.0)))  # largest |g| / scale just below float16's maximum
        arrays[f"{name}/grad"] = (g / scale).astype(np.float16)
        arrays[f"{name}/scale"] = np.array(scale)
        arrays[f"{name}/loss"] = np.array(loss.item())
        print(f"  {name}: loss {loss.item():.6f}, |dx| max {np.abs(g).max():.3e}, norm {np.linalg.norm(g):.3e}, scale 2^{int(np.log2(scale))}")
        cases.append(dict(name=name, cfg=cfg, mapper=mapper, chunk=chunk, training_chunks=tchunks, new_channel_init=init, n_channels=n_ch, img=img,
                          H=H, W=W, num_classes=K, B=B, train=train, seed=seed, batch_seed=bseed, rows=rows))
    mg.save("input_grad", dict(cases=cases), arrays)


if __name__ == "__main__":
    main()
