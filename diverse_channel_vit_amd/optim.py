"""Fused AdamW over the model's flat parameter/gradient arenas.

Restates what the reference builds with ``make_my_optimizer('adamw', ...)`` -> timm AdamW
(optimizers.py:20-21, trainer.py:1224-1230): decoupled weight decay on every parameter that has a
gradient, bias-corrected Adam.  lr and weight_decay are read from ``param_groups`` every step, so the
reference's per-epoch LR scheduler and per-step weight-decay schedule (trainer.py:1009-1019) drive it unchanged.

ONE parameter group, every encoder parameter's ``.grad`` aliasing the model's gradient arena (the reference's
training from scratch, the normal zero_grad(set_to_none=True) -> backward flow): the whole encoder (≈99.7 % of
the parameters) is updated by ONE launch over one contiguous range (dcv_adamw / dcv_adamw_dyn).

SEVERAL groups (up to DCV_ADAMW_MAX_GROUPS: the DINO decay / no-decay split, layer-wise learning-rate decay —
``param_groups()``), or encoder parameters that sit the step out (``model.freeze_prefix()``, any
``requires_grad_(False)``): still ONE launch over the encoder range, dcv_adamw_groups with a table of runs
(``build_segments``), every run naming its group's row of scalars in a device table, or -1: not touched.  The few
parameters outside the encoder range take one launch each.  Parameters whose grad is None are skipped and get no
state, exactly like torch/timm AdamW; step counts are kept per group."""
from __future__ import annotations

import torch

from . import hip


_NO_DECAY_TABLES = ("feature_extractor.cls_token", "feature_extractor.pos_embed", "feature_extractor.patch_embed.channel_embed.weight")


def param_groups(model, lr, weight_decay, layer_decay=1.0, no_decay_1d=True):
    """Parameter groups for fine-tuning a DiChaViT (HipAdamW or any torch optimizer).
    Layer ids (dichavit.layer_id_of): 0 = tokeniser projection, cls_token, positional and channel embeddings, channel proxies; i + 1 =
    block i; depth + 1 = final norm, head, `proxies`.  A group's lr is lr * layer_decay ** (depth + 1 - id), the factor also stored as
    ``lr_scale`` (layer-wise learning-rate decay; 1.0: one lr).  no_decay_1d: parameters with ndim <= 1 (biases, LayerNorm) and the
    embedding / token tables (cls_token, pos_embed, channel_embed) get weight_decay = 0, the DINO split.  REGULARISED groups come first, by
    ascending layer id, then the others: with layer_decay = 1 that is the two-group split whose group 0 is the only regularised one — the
    group the reference trainer's weight-decay schedule writes to (trainer.py:1012-1013).  Only parameters that require a gradient are
    listed; empty groups are dropped.  Each group also names its ``layer_id`` (None when layers are not separated)."""
    from .dichavit import layer_id_of
    depth = len(model.feature_extractor.blocks)
    split = float(layer_decay) != 1.0
    buckets = {}
    for name, p in model.named_parameters():  # shared parameters (adaptive_interface.0 = proxies) come once
        if not p.requires_grad:
            continue
        lid = layer_id_of(name, depth)
        plain = bool(no_decay_1d) and (p.ndim <= 1 or name in _NO_DECAY_TABLES)
        buckets.setdefault((plain, lid if split else None), []).append(p)
    groups = []
    for (plain, lid), ps in sorted(buckets.items(), key=lambda kv: (kv[0][0], -1 if kv[0][1] is None else kv[0][1])):
        scale = float(layer_decay) ** (depth + 1 - lid) if split else 1.0
        groups.append(dict(params=ps, lr=lr * scale, weight_decay=0.0 if plain else weight_decay, lr_scale=scale, layer_id=lid))
    return groups


def build_segments(offsets, total, rows):
    """The run table of dcv_adamw_groups, on the host.  offsets[i]: first float of tensor i's arena slot (ascending, multiples of 4, the
    first one 0); total: floats of the range (a multiple of 4); rows[i]: the hyper-parameter row tensor i takes, or -1 when it does not
    take part.  Tensor i owns [offsets[i], offsets[i + 1]) — its padding floats belong to it, hence to the run it is in.  Adjacent tensors
    of one row merge.  Returns (ends4, groups): run s is [ends4[s - 1], ends4[s]) in float4 units, sorted, covering [0, total / 4)."""
    if not offsets or offsets[0] != 0 or total % 4 or any(o % 4 for o in offsets) or len(rows) != len(offsets):
        raise ValueError("arena slots must start at 0, be 16-byte aligned and come with one row each")
    ends4, groups = [], []
    for i, (o, r) in enumerate(zip(offsets, rows)):
        end = offsets[i + 1] if i + 1 < len(offsets) else total
        if end <= o:
            raise ValueError("arena slots must be ascending and non-empty")
        if groups and groups[-1] == r:
            ends4[-1] = end // 4
        else:
            ends4.append(end // 4)
            groups.append(int(r))
    return ends4, groups


class HipAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, model=None, capturable=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        if len(self.param_groups) > hip.ADAMW_MAX_GROUPS:
            raise ValueError(f"HipAdamW takes at most {hip.ADAMW_MAX_GROUPS} parameter groups (DCV_ADAMW_MAX_GROUPS)")
        self.model = model
        self._gsteps = [0] * len(self.param_groups)  # one step count per group (bias corrections): a group advances when one of its parameters is updated
        self._m = self._v = None
        # capturable: the kernels read {lr, betas, eps, wd, bias corrections} from a device buffer that advance()
        # rewrites before every step, so step() can live inside a captured HIP graph (graph.GraphedTrainStep)
        self.capturable = capturable
        self._hyper_dev = None  # [groups][8]: dcv_adamw_set_hyper's row per group
        self._part = None       # capturable: ids of the parameters that required a gradient at advance()
        self._seg_key = self._seg_dev = None

    @property
    def _step(self):
        return max(self._gsteps)

    @_step.setter
    def _step(self, value):
        self._gsteps = [int(value)] * len(self.param_groups)

    def _hyper(self, device):
        n = 8 * len(self.param_groups)
        if self._hyper_dev is None or self._hyper_dev.numel() != n or self._hyper_dev.device != device:
            self._hyper_dev = torch.zeros(n, dtype=torch.float32, device=device)
        return self._hyper_dev

    def _upload_rows(self, device):
        rows = [(float(g["lr"]), g["betas"][0], g["betas"][1], float(g["eps"]), float(g["weight_decay"])) for g in self.param_groups]
        hip.adamw_set_hyper_groups(self._hyper(device), rows, [max(s, 1) for s in self._gsteps], 1.0)  # a group that never advanced is in no run

    def advance(self):
        """capturable mode: bump the step counts and hand this step's scalars to the device.  They travel BY VALUE as the
        arguments of a small kernel on the current stream (dcv_adamw_set_hyper, dcv_adamw_set_hyper_groups): stream-ordered against
        the replays, and there is no host staging buffer that a host running several steps ahead of the device could overwrite.
        A parameter takes part in the coming step if it requires a gradient NOW (the captured step cannot change that later); a group
        advances if one of its parameters does."""
        groups = self.param_groups
        if len(self._gsteps) != len(groups):
            self._gsteps += [0] * (len(groups) - len(self._gsteps))
        self._part = {id(p) for g in groups for p in g["params"] if p.requires_grad}
        dev = groups[0]["params"][0].device
        if len(groups) == 1:
            grp = groups[0]
            self._gsteps[0] += 1
            b1, b2 = grp["betas"]
            hip.adamw_set_hyper(self._hyper(dev), float(grp["lr"]), b1, b2, float(grp["eps"]), float(grp["weight_decay"]), self._gsteps[0], 1.0)
            return
        for gi, g in enumerate(groups):
            if any(id(p) in self._part for p in g["params"]):
                self._gsteps[gi] += 1
        self._upload_rows(dev)

    def _ensure_state(self):
        model = self.model
        arena = model._arena
        if self._m is None or self._m.shape != arena.shape or self._m.device != arena.device:
            self._m = torch.zeros_like(arena)
            self._v = torch.zeros_like(arena)
            self._bound = set()
            self._off = {id(p): o for p, o in zip(model._all_params, model._all_off)}
            self._seg_key = self._seg_dev = None
            for p in model._all_params:
                if p in self.state and "exp_avg" in self.state[p]:  # moments that load_state_dict() put there (a resumed run)
                    self._bind(p, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"])

    def _bind(self, p, m_src=None, v_src=None):
        """state[p] = views into the flat moment arenas.  Done lazily, for parameters that actually get updated — like
        torch/timm AdamW, parameters that never receive a gradient (``proxies`` in CE mode, frozen parameters) have no optimizer
        state, so state_dict() has the reference's layout (trainer.py:1296)."""
        o = self._off[id(p)]
        mv, vv = self._m[o:o + p.numel()].view(p.shape), self._v[o:o + p.numel()].view(p.shape)
        if m_src is not None:
            mv.copy_(m_src)
            vv.copy_(v_src)
        st = self.state[p]
        st["exp_avg"], st["exp_avg_sq"] = mv, vv
        self._bound.add(id(p))

    def load_state_dict(self, state_dict):
        """Accepts torch.optim.AdamW / timm AdamW layouts ("optimizer_params" of the reference's checkpoints, trainer.py:1321):
        per-parameter exp_avg / exp_avg_sq / step, indexed in model.parameters() order.  The moments are copied into the
        flat arenas at the next step; each group's step count (bias corrections) continues from its parameters' loaded value."""
        super().load_state_dict(state_dict)
        self._gsteps = []
        for g in self.param_groups:
            steps = [int(self.state[p]["step"]) for p in g["params"] if p in self.state and "step" in self.state[p]]
            self._gsteps.append(max(steps) if steps else 0)
        self._m = self._v = None

    def _segments(self, model, rows):
        """Device copy of the run table for this membership / participation (rebuilt only when either changes)."""
        key = (model._arena.data_ptr(), tuple(rows))
        if self._seg_key != key:
            ends4, grps = build_segments(model._enc_off, model._enc_size, rows)
            if len(ends4) > hip.ADAMW_MAX_SEGS:
                raise RuntimeError(f"{len(ends4)} runs of parameter groups in the arena: more than DCV_ADAMW_MAX_SEGS = {hip.ADAMW_MAX_SEGS}")
            dev = model._arena.device
            self._seg_dev = (torch.tensor(ends4, dtype=torch.int32, device=dev), torch.tensor(grps, dtype=torch.int32, device=dev), len(ends4))
            self._seg_key = key
        return self._seg_dev

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        model = self.model
        if model is None or model._arena is None:
            raise RuntimeError("HipAdamW needs the arena-backed DiChaViT it optimises (pass model=...) after its first forward")
        if model._dp is not None:
            model._dp.finalize()
        self._ensure_state()
        groups = self.param_groups
        if len(groups) > hip.ADAMW_MAX_GROUPS:
            raise ValueError(f"HipAdamW takes at most {hip.ADAMW_MAX_GROUPS} parameter groups (DCV_ADAMW_MAX_GROUPS)")
        if len(self._gsteps) != len(groups):  # add_param_group() after construction
            self._gsteps += [0] * (len(groups) - len(self._gsteps))
        if self.capturable and (self._hyper_dev is None or self._part is None):
            raise RuntimeError("capturable HipAdamW: call advance() before step()")
        ga = model._grad_arena
        enc = model._enc_params
        if len(groups) == 1:
            mine = {id(p) for p in groups[0]["params"]}
            fused = ga is not None and all(
                id(p) in mine and p.grad is not None and p.grad.data_ptr() == ga.data_ptr() + o * 4
                for p, o in zip(enc, model._enc_off))
            if fused:
                return self._step_single(model, ga, loss, True)
        # parameter groups, or encoder parameters that sit this step out (frozen, no gradient): the run table
        part = self._part if self.capturable else None
        takes = (lambda p: p.grad is not None and id(p) in part) if part is not None else (lambda p: p.grad is not None)  # noqa: E731
        gid = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
        rows, table_ok = [], ga is not None
        for p, o in zip(enc, model._enc_off):
            gi = gid.get(id(p))
            if gi is None or not takes(p):
                rows.append(-1)
                continue
            rows.append(gi)
            table_ok = table_ok and p.grad.data_ptr() == ga.data_ptr() + o * 4
        table_ok = table_ok and any(r >= 0 for r in rows)
        if len(groups) == 1 and not table_ok:
            return self._step_single(model, ga, loss, False)  # gradients outside the arena: one launch per tensor, as ever
        if not self.capturable:
            for gi, g in enumerate(groups):
                if any(takes(p) for p in g["params"]):
                    self._gsteps[gi] += 1
            self._upload_rows(model._arena.device)
        hyper = self._hyper_dev
        done = set()
        if table_ok:
            ends4, grps, n_seg = self._segments(model, rows)
            hip.adamw_groups(model._arena, ga, self._m, self._v, model._enc_size, ends4, grps, n_seg, hyper, len(groups))
            done = {id(p) for p in enc}
        for gi, g in enumerate(groups):
            for p in g["params"]:
                if not takes(p):
                    continue
                if id(p) not in done:
                    gr = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    o = self._off.get(id(p))
                    if o is None:
                        raise RuntimeError("parameter is not part of the model's arena")
                    n = p.numel()
                    if (o * 4) % 16 or gr.data_ptr() % 16:
                        raise RuntimeError("unaligned parameter slot")
                    hip.adamw_dyn(model._arena[o:o + n], gr, self._m[o:o + n], self._v[o:o + n], n, hyper[8 * gi:8 * gi + 8])
                if id(p) not in self._bound:
                    self._bind(p)
                self.state[p]["step"] = self._gsteps[gi]
        return loss

    def _step_single(self, model, ga, loss, fused):
        """ONE group.  fused — every encoder gradient sits in the arena: dcv_adamw / dcv_adamw_dyn over the whole encoder range and one
        launch per tensor outside it; otherwise (gradients that do not alias the arena) one launch per tensor."""
        grp = self.param_groups[0]
        lr, (b1, b2), eps, wd = float(grp["lr"]), grp["betas"], float(grp["eps"]), float(grp["weight_decay"])
        if not self.capturable:
            self._gsteps[0] += 1
        step = self._gsteps[0]
        enc = model._enc_params
        done = set()
        if fused:
            n = model._enc_size
            if self.capturable:
                hip.adamw_dyn(model._arena, ga, self._m, self._v, n, self._hyper_dev)
            else:
                hip.adamw(model._arena, ga, self._m, self._v, n, lr, b1, b2, eps, wd, step, 1.0)
            done = {id(p) for p in enc}
        off = self._off
        for p in grp["params"]:
            if id(p) in done or p.grad is None:
                continue
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            o = off.get(id(p))
            if o is None:
                raise RuntimeError("parameter is not part of the model's arena")
            n = p.numel()
            if (o * 4) % 16 or g.data_ptr() % 16:
                raise RuntimeError("unaligned parameter slot")
            if self.capturable:
                hip.adamw_dyn(model._arena[o:o + n], g, self._m[o:o + n], self._v[o:o + n], n, self._hyper_dev)
            else:
                hip.adamw(model._arena[o:o + n], g, self._m[o:o + n], self._v[o:o + n], n, lr, b1, b2, eps, wd, step, 1.0)
        for p in grp["params"]:
            if p.grad is None:
                continue
            if id(p) not in self._bound:
                self._bind(p)
            self.state[p]["step"] = step
        return loss


@torch.no_grad()
def clip_grad_norm_(model, max_norm: float) -> torch.Tensor:
    """trainer.py:1003-1004 -> torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) (L2) for the arena-backed model:
    one sum-of-squares launch per run of gradients in the encoder's gradient arena (ONE when every encoder parameter has a gradient,
    two with a frozen prefix) plus one per small parameter outside it, then every
    gradient is multiplied by min(1, max_norm / (total_norm + 1e-6)).  The coefficient never leaves the device (no host
    sync; capturable).  Returns the total norm as a 0-d device tensor, like torch.  Under DataParallel the pending
    all-reduces are awaited first, so the norm is that of the averaged gradient on every rank."""
    if model._dp is not None:
        model._dp.finalize()
    ga = model._grad_arena
    enc = model._enc_params
    bufs = []
    seen = set()
    if ga is not None:
        # merged runs of arena-resident gradients (slot padding included: it holds zeros): one run when every encoder parameter has its
        # gradient there, two with a frozen prefix, one per run of trainable tensors under set_trainable().  The slot of a parameter WITHOUT
        # .grad stays out (under a DataParallel reducer a frozen weight still has its gradient computed into the arena).
        offs, total = model._enc_off, model._enc_size
        start = end = None
        for i, (p, o) in enumerate(zip(enc, offs)):
            if p.grad is None or p.grad.data_ptr() != ga.data_ptr() + o * 4:
                continue
            seen.add(id(p))
            nxt = offs[i + 1] if i + 1 < len(offs) else total
            if end == o:
                end = nxt
            else:
                if start is not None:
                    bufs.append((ga[start:end], end - start))
                start, end = o, nxt
        if start is not None:
            bufs.append((ga[start:end], end - start) if (start, end) != (0, total) else (ga, total))
    for p in model.parameters():
        if id(p) in seen or p.grad is None:
            continue
        seen.add(id(p))
        g = p.grad
        if not g.is_contiguous() or g.dtype != torch.float32 or g.data_ptr() % 16:
            p.grad = g = g.contiguous().float().clone()
        bufs.append((g, g.numel()))
    if not bufs:
        return torch.zeros((), device=model._arena.device if model._arena is not None else "cpu")
    acc = getattr(model, "_clip_acc", None)
    if acc is None or acc.device != bufs[0][0].device:
        acc = model._clip_acc = torch.zeros(1, dtype=torch.float32, device=bufs[0][0].device)
    acc.mul_(0.0)  # a kernel, not a memset node (memset nodes did not replay correctly inside captured graphs)
    for g, n in bufs:
        hip.sumsq_acc(g, n, acc)
    for g, n in bufs:
        hip.clip_scale(g, n, acc, max_norm)
    return acc.sqrt().reshape(())
