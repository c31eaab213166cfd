"""The train step's switches, crossed pairwise: the factor table, the covering-array generator with its frozen rows, and the runners (fp64 oracle,
HIP model, plain twin, pass-through launch recorder, comparator) that tests/test_switch_pairs_cpu.py, tests/test_switch_pairs_gpu.py and
tools/switch_pairs_profile.py share.  No test functions here.

Every pair of levels of two different factors that the constraints allow appears together in at least one row of ROWS.  That is all pair
coverage promises: a defect that needs three particular levels at once can still pass.

Shapes: patch 8, a 32-px model (4 x 4 positional grid), images of 32 px (n = 16 patches per channel) or 48 px (n = 36, grid resampled), 6 channels
in the mapper, batch 3, 7 classes.  N = 1 + C n is 17 / 37 / 49 (< 64), 97 / 109 (64 .. 128) and 217 (> 128) before token dropout: both sides of the
attention forward's 64-key and 128-query tiles.  DEPTH stays at the reference's 12 blocks — nothing is patched: a row with its twelve-block fp64
oracle takes about a second, so the bounds are met with the error twelve blocks accumulate, DropPath's rates are the real linspace(0, 0.4, 12) and a
frozen prefix ends in the middle (k = 6) or right under the last block (k = 11)."""
import inspect
import itertools
import random
import time

import numpy as np
import torch

from oracle import dichavit_oracle as orc

DEPTH = orc.MODEL_SIZES["small"][1]  # 12, tiny and small alike
PATCH, MODEL_IMG, OTHER_IMG, N_CHANNELS, BATCH, NUM_CLASSES = 8, 32, 48, 6, 3, 7
PICKED = {1: [2], 3: [4, 1, 5], 6: [0, 1, 2, 3, 4, 5]}  # the pinned HCS draw per level of `channels`: global ids, in this order
LAMBDA_ORTHO, LAMBDA_PROXY = 0.1, 0.1
MAX_ROWS = 24
SEED = 29

# ---------------------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------------------
FACTORS = (
    ("width", ("tiny", "small")),                                   # A: D 192 / 3 heads, D 384 / 6 heads
    ("channels", (1, 3, 6)),                                        # B: channels in the step, pinned with hcs_sampler (PICKED)
    ("token_drop", ("none", "token_random50", "channel")),          # C: cfg.dropout_tokens_hcs
    ("drop_path", (0.0, 0.4)),                                      # D: cfg.drop_path_rate, masks pinned with drop_path_sampler
    ("losses", ("none", "ortho", "ortho_proxy_fused", "ortho_proxy_unfused")),  # E: the extra losses; fused / torch proxy term
    ("channel_embed", (True, False)),                               # F: cfg.use_channelvit_channels
    ("input", ("float", "float_resized", "uint8")),                 # G: fp32 at 32 px, fp32 at 48 px, uint8 + set_input_normalisation
    ("grads", ("all", "freeze_prefix", "input")),                   # H: what gets a gradient
    ("passes", (1, 2)),                                             # I: backward passes before the comparison
    ("prescaled", (True, False)),                                   # J: model.attn_prescaled
    ("fuse_ln", ("forced", "off")),                                 # K: fuse_ln_fwd=True with fuse_ln_min_tiles=0 / fuse_ln_fwd=False
    ("cls_tail", (True, False)),                                    # L: model.cls_only_tail
    ("wgrad", ("grouped_private", "ungrouped_shared", "grouped_stream")),  # M: wgrad_group / wgrad_private_scratch / wgrad_stream
    ("reductions", ("deterministic", "atomic")),                    # N: hip.set_deterministic
    ("copies", ("nearest", "stochastic")),                          # O: model.stochastic_weight_rounding
)
NAMES = tuple(f for f, _ in FACTORS)
LEVELS = dict(FACTORS)

# What cannot be crossed, as predicates over a (possibly partial) {factor: level} mapping; every one involves two factors.
EXCLUDES = (
    ("the proxy term reads channel_embed, which the no-channel-embedding mode does not have",
     lambda r: r.get("channel_embed") is False and r.get("losses") in ("ortho_proxy_fused", "ortho_proxy_unfused")),
    ("the LayerNorm epilogue exists for D = 384 only: with tiny, `forced` is the `off` level",
     lambda r: r.get("width") == "tiny" and r.get("fuse_ln") == "forced"),
    ("the grouped weight-gradient launch takes 384-row tiles (_group_ok): with tiny, the grouped levels launch one by one",
     lambda r: r.get("width") == "tiny" and r.get("wgrad") in ("grouped_private", "grouped_stream")),
    ("uint8 images get no gradient",
     lambda r: r.get("grads") == "input" and r.get("input") == "uint8"),
    ("one channel: ceil(0.5 * 1) = 1 keeps everything in the reference's bookkeeping, and the model refuses the ill-defined mask",
     lambda r: r.get("channels") == 1 and r.get("token_drop") not in (None, "none")),
)

# Attributes the rows set on a constructed model, with the defaults they have when no DCV_* environment variable is set.
SWITCH_DEFAULTS = dict(attn_prescaled=True, fuse_ln_fwd=True, fuse_ln_min_tiles=96, cls_only_tail=True, wgrad_group=True,
                       wgrad_private_scratch=True, wgrad_stream=False, fused_proxy_loss=True, stochastic_weight_rounding=True,
                       hcs_sampler=None, drop_path_sampler=None)
SWITCH_ENV = ("DCV_ATTN_PS", "DCV_FUSE_LN", "DCV_FUSE_LN_MIN_TILES", "DCV_CLS_TAIL", "DCV_WGRAD_GROUP", "DCV_WGRAD_PRIVATE", "DCV_WGRAD_STREAM",
              "DCV_FUSED_PROXY_LOSS", "DCV_WEIGHT_ROUNDING")
PLAIN = dict(prescaled=False, fuse_ln="off", cls_tail=False, wgrad="ungrouped_shared", reductions="deterministic", copies="nearest")


def allowed(r):
    return not any(pred(r) for _, pred in EXCLUDES)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the covering array
# ---------------------------------------------------------------------------------------------------------------------------------------------
def pairs_of(levels):
    """the pairs a row (tuple of levels in FACTORS order) holds, as (factor index, level index, factor index, level index)"""
    ix = [LEVELS[f].index(v) for f, v in zip(NAMES, levels)]
    return {(i, ix[i], j, ix[j]) for i in range(len(ix)) for j in range(i + 1, len(ix))}


def allowed_pairs():
    """every pair of levels of two different factors that some allowed row holds"""
    constrained = [f for f in NAMES if any(pred({f: v, g: w}) for _, pred in EXCLUDES for v in LEVELS[f] for g in NAMES if g != f for w in LEVELS[g])]
    out = set()
    for i, j in itertools.combinations(range(len(NAMES)), 2):
        rest = [f for f in constrained if f not in (NAMES[i], NAMES[j])]
        for li, lj in itertools.product(range(len(FACTORS[i][1])), range(len(FACTORS[j][1]))):
            fixed = {NAMES[i]: FACTORS[i][1][li], NAMES[j]: FACTORS[j][1][lj]}
            if any(allowed({**fixed, **dict(zip(rest, combo))}) for combo in itertools.product(*(LEVELS[f] for f in rest))):
                out.add((i, li, j, lj))
    return out


def _candidate(rng, todo):
    i, li, j, lj = rng.choice(sorted(todo))
    ix = {i: li, j: lj}
    order = [k for k in range(len(NAMES)) if k not in ix]
    rng.shuffle(order)
    for k in order:
        best, best_gain = [], -1
        for lk in range(len(FACTORS[k][1])):
            if not allowed({NAMES[m]: FACTORS[m][1][lm] for m, lm in {**ix, k: lk}.items()}):
                continue
            gain = sum(((min(k, m), (lk, lm)[k > m], max(k, m), (lm, lk)[k > m]) in todo) for m, lm in ix.items())
            if gain > best_gain:
                best, best_gain = [lk], gain
            elif gain == best_gain:
                best.append(lk)
        if not best:
            return None
        ix[k] = rng.choice(best)
    return tuple(FACTORS[k][1][ix[k]] for k in range(len(NAMES)))


def generate(seed=SEED, tries=40):
    """greedy pairwise covering array (AETG-style): each new row is the best of `tries` candidates, a candidate starts from an uncovered pair and
    gives every other factor, in random order, the allowed level that covers the most uncovered pairs with the factors set so far"""
    rng = random.Random(seed)
    todo, rows = allowed_pairs(), []
    while todo:
        cands = [c for c in (_candidate(rng, todo) for _ in range(tries)) if c is not None]
        best = max(cands, key=lambda c: len(pairs_of(c) & todo))
        rows.append(best)
        todo -= pairs_of(best)
    return rows


# generate() frozen: a change of the generator cannot move the rows silently (test_switch_pairs_cpu.py compares the two)
ROWS = (
    ('tiny', 6, 'token_random50', 0.0, 'ortho', True, 'float_resized', 'all', 2, True, 'off', False, 'ungrouped_shared', 'atomic', 'stochastic'),
    ('small', 3, 'channel', 0.4, 'none', False, 'float_resized', 'input', 1, False, 'forced', True, 'grouped_private', 'deterministic', 'nearest'),
    ('small', 1, 'none', 0.4, 'ortho_proxy_unfused', True, 'float', 'freeze_prefix', 2, True, 'off', True, 'grouped_stream', 'deterministic', 'nearest'),
    ('small', 1, 'none', 0.0, 'ortho', False, 'uint8', 'freeze_prefix', 1, False, 'forced', False, 'grouped_private', 'atomic', 'stochastic'),
    ('tiny', 3, 'channel', 0.0, 'ortho_proxy_fused', True, 'float', 'input', 1, False, 'off', False, 'ungrouped_shared', 'atomic', 'nearest'),
    ('small', 6, 'token_random50', 0.4, 'ortho_proxy_fused', True, 'uint8', 'all', 1, False, 'forced', True, 'grouped_stream', 'deterministic', 'stochastic'),
    ('tiny', 3, 'channel', 0.4, 'none', False, 'uint8', 'freeze_prefix', 2, True, 'off', False, 'ungrouped_shared', 'deterministic', 'stochastic'),
    ('small', 6, 'token_random50', 0.0, 'none', False, 'float', 'input', 2, True, 'forced', True, 'grouped_stream', 'atomic', 'nearest'),
    ('tiny', 1, 'none', 0.4, 'ortho_proxy_unfused', True, 'float_resized', 'input', 1, True, 'off', True, 'ungrouped_shared', 'atomic', 'stochastic'),
    ('small', 6, 'channel', 0.0, 'ortho_proxy_unfused', True, 'uint8', 'all', 2, False, 'forced', False, 'grouped_private', 'deterministic', 'nearest'),
    ('small', 3, 'none', 0.4, 'ortho', False, 'float', 'all', 1, True, 'off', True, 'grouped_private', 'deterministic', 'stochastic'),
    ('small', 6, 'none', 0.4, 'ortho_proxy_fused', True, 'float_resized', 'freeze_prefix', 2, True, 'forced', True, 'ungrouped_shared', 'deterministic', 'stochastic'),
    ('small', 3, 'channel', 0.0, 'ortho', False, 'float_resized', 'input', 2, True, 'off', False, 'grouped_stream', 'deterministic', 'nearest'),
    ('small', 3, 'token_random50', 0.4, 'ortho_proxy_unfused', True, 'float', 'freeze_prefix', 1, False, 'forced', True, 'grouped_private', 'atomic', 'nearest'),
    ('tiny', 1, 'none', 0.0, 'none', True, 'uint8', 'all', 2, True, 'off', False, 'ungrouped_shared', 'deterministic', 'stochastic'),
    ('small', 1, 'none', 0.4, 'ortho_proxy_fused', True, 'float_resized', 'input', 1, True, 'forced', False, 'grouped_private', 'atomic', 'stochastic'),
)


class Row:
    """One row with everything derived from it: the configuration, the pinned random draws and the inputs of each pass."""

    def __init__(self, index, levels, twin=False, freeze_k=None):
        self.index, self.levels, self.twin = index, tuple(levels), twin
        self.__dict__.update(zip(NAMES, levels))
        self.id = f"r{index:02d}" + ("-twin" if twin else "")
        self.small = self.width == "small"
        self.img = OTHER_IMG if self.input == "float_resized" else MODEL_IMG
        self.picked = PICKED[self.channels]
        self.n = (self.img // PATCH) ** 2
        self.N_full = 1 + self.channels * self.n
        self.freeze_k = freeze_k if twin else self._freeze_k()
        self.lam_o = LAMBDA_ORTHO if self.losses != "none" else 0.0
        self.lam_p = LAMBDA_PROXY if self.losses.startswith("ortho_proxy") else 0.0
        self.cfg = dict(name="dichavit", pretrained_model_name=self.width, patch_size=PATCH, temperature=0.07, learnable_temp=False,
                        enable_sample=True, use_channelvit_channels=self.channel_embed, orthogonal_channel_emb_init=True,
                        dropout_tokens_hcs=self.token_drop, freeze_channel_emb=False, block_type="block", hcs_sampling="none",
                        hcs_sampling_temp=0.1, proxy_loss_lambda=self.lam_p, ortho_loss_v1_lambda=self.lam_o, drop_path_rate=self.drop_path,
                        gamma_s=0.5, gamma_d=4.0, reverse_pos_pairs=True, use_square=False)
        self.seed = self._seed()
        self.keeps = self._keeps(self.seed)
        self.N = [self.N_full if k is None else len(k) for k in self.keeps]  # tokens the encoder sees, per pass

    def _freeze_k(self):
        """freeze_prefix's k: the middle (6) on even rows, right under the last block (11) on odd ones -- but a row with a grouped weight-gradient
        level and the CLS tail takes the middle, since the CLS-only tail launches its products one by one (no plan, no private scratch) and a
        backward of block 11 alone would leave the row's weight-gradient level without effect.  The twin keeps its row's k."""
        if self.grads != "freeze_prefix":
            return None
        if self.cls_tail and self.wgrad != "ungrouped_shared":
            return DEPTH // 2
        return (DEPTH // 2, DEPTH - 1)[self.index % 2]

    def plain_twin(self):
        d = dict(zip(NAMES, self.levels), **PLAIN)
        if d["losses"] == "ortho_proxy_fused":
            d["losses"] = "ortho_proxy_unfused"
        return Row(self.index, tuple(d[f] for f in NAMES), twin=True, freeze_k=self.freeze_k)

    def describe(self):
        return " ".join(f"{f}={v}" for f, v in zip(NAMES, self.levels))

    # --- the pinned draws -------------------------------------------------------------------------------------------------------------------
    def _keeps(self, seed):
        rng = random.Random(seed)  # the model draws from the global python RNG, seeded with the same number before the first forward
        return [orc.token_keep(self.token_drop, self.channels, self.n, rng) for _ in range(self.passes)]

    def _seed(self):
        """the first seed from 1000 * index whose token-dropout draws keep CLS, at least two other tokens and fewer than all, in every pass"""
        for s in itertools.count(1000 * self.index + 7):
            if all(k is None or (k[0] == 0 and 3 <= len(k) < self.N_full) for k in self._keeps(s)):
                return s

    def drop_masks(self, p):
        """DropPath keep masks [B] of pass p in the oracle's order (block 1 attention, block 1 MLP, block 2 ...; block 0 never drops): sample 0 is
        kept everywhere, sample 1 is dropped in the last block's attention branch, the rest is a seeded draw."""
        if self.drop_path == 0.0:
            return None
        m = (np.random.RandomState(self.seed * 10 + p).uniform(size=(2 * (DEPTH - 1), BATCH)) < 0.6).astype(np.float64)
        m[:, 0] = 1.0
        m[-2, 1] = 0.0
        return [torch.from_numpy(r.copy()) for r in m]

    def drop_sampler(self, p):
        masks = self.drop_masks(p)
        return None if masks is None else (lambda bi, branch, B, dev: masks[2 * (bi - 1) + (branch == "mlp")].float())

    # --- inputs -----------------------------------------------------------------------------------------------------------------------------
    def normalisation(self):
        rs = np.random.RandomState(5)
        return rs.uniform(0.02, 0.3, N_CHANNELS).astype(np.float32), rs.uniform(0.05, 0.2, N_CHANNELS).astype(np.float32)

    def batch(self, p):
        """(what the model is fed, the normalised fp32 images the reference would see, labels) of pass p"""
        x, y = orc.make_batch(self.seed * 10 + p, BATCH, N_CHANNELS, self.img, NUM_CLASSES)
        if self.input != "uint8":
            return x, x, y
        mean, std = self.normalisation()
        raw = torch.from_numpy(np.random.RandomState(self.seed * 10 + p).randint(0, 256, (BATCH, N_CHANNELS, self.img, self.img)).astype(np.uint8))
        ref_in = (raw.float() / 255.0 - torch.from_numpy(mean)[None, :, None, None]) / torch.from_numpy(std)[None, :, None, None]
        return raw, ref_in, y

    def trains(self, name):
        """does this row train the parameter `name` (a named_parameters() / state-dict key)"""
        if self.freeze_k is None:
            return True
        if name.startswith("feature_extractor.blocks."):
            return int(name.split(".")[2]) >= self.freeze_k
        return not name.startswith("feature_extractor.") or name.startswith("feature_extractor.norm.")

    def backward_blocks(self):
        return DEPTH - (self.freeze_k or 0)

    def grouped_blocks(self):
        """blocks of the backward that take the grouped weight-gradient launch: all of them but the CLS-only tail, which launches its products one
        by one on the main stream"""
        return self.backward_blocks() - (1 if self.cls_tail else 0)


def rows():
    return [Row(i, lv) for i, lv in enumerate(ROWS)]


class Cfg(dict):
    __getattr__ = dict.get


def new_model(row):
    import diverse_channel_vit_amd as dcv
    cfg = Cfg(row.cfg, in_channel_names=[f"c{i}" for i in range(N_CHANNELS)], img_size=[MODEL_IMG], num_classes=NUM_CLASSES)
    return dcv.dichavit(cfg, mapper={"train": list(range(N_CHANNELS))})


def state(row, dtype):
    return orc.make_state(orc.state_shapes(row.cfg, N_CHANNELS, MODEL_IMG, NUM_CLASSES), row.seed, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------
def run_oracle(row):
    """fp64: per pass loss, extra term and logits; the gradient of the summed losses for every state tensor; per pass the input gradient where
    the row asks for it; the eval forward (all channels, no drop of any kind) of the first pass's batch."""
    sd = state(row, torch.float64)
    for k, v in sd.items():
        v.requires_grad_(row.trains(k))  # a frozen tensor gets no gradient here either
    idx = row.picked  # the mapper lists the global ids 0 .. 5 in order: position == id
    out, xs, total = dict(loss=[], extra=[], logits=[]), [], 0.0
    for p in range(row.passes):
        _, ref_in, y = row.batch(p)
        x = ref_in.double()
        if row.grads == "input":
            x.requires_grad_(True)
        xs.append(x)
        loss, _, extra, logits = orc.train_loss(sd, x, y, row.cfg, row.picked, idx, keep=row.keeps[p], drop_masks=row.drop_masks(p))
        total = total + loss
        out["loss"].append(loss.item()); out["extra"].append(extra.item()); out["logits"].append(logits.detach())
    total.backward()
    out["grads"] = {k: (None if v.grad is None else v.grad.detach()) for k, v in sd.items()}
    out["xgrads"] = [x.grad.detach() for x in xs] if row.grads == "input" else None
    with torch.no_grad():
        allc = list(range(N_CHANNELS))
        out["eval"] = orc.forward({k: v.detach() for k, v in sd.items()}, row.batch(0)[1].double(), row.cfg, allc, allc)[0]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------------------
def set_switches(model, row):
    model.attn_prescaled = row.prescaled
    model.fuse_ln_fwd = row.fuse_ln == "forced"
    model.fuse_ln_min_tiles = 0 if row.fuse_ln == "forced" else SWITCH_DEFAULTS["fuse_ln_min_tiles"]
    model.cls_only_tail = row.cls_tail
    model.wgrad_group = model.wgrad_private_scratch = row.wgrad != "ungrouped_shared"
    model.wgrad_stream = row.wgrad == "grouped_stream"
    model.fused_proxy_loss = row.losses != "ortho_proxy_unfused"
    model.stochastic_weight_rounding = row.copies == "stochastic"
    picked = row.picked
    model.hcs_sampler = lambda m, chunk, cur: (list(picked), [cur.index(c) for c in picked])


EVAL_MARK = "<model.eval()>"  # what run_model puts into a recorder's log between the training passes and the eval forward


def run_model(row, device, log=None):
    """the same passes on the HIP path, then one eval forward; returns what run_oracle returns (fp64, on the host).  log: a recorder's log, which
    gets EVAL_MARK where the training passes end"""
    from diverse_channel_vit_amd import hip
    t0 = time.perf_counter()
    model = new_model(row)
    st = state(row, torch.float32)
    assert set(model.state_dict()) - {"adaptive_interface.0"} == set(st)
    model.load_state_dict({**st, "adaptive_interface.0": st["proxies"]}, strict=True)
    model = model.to(device).train()
    set_switches(model, row)
    if row.input == "uint8":
        model.set_input_normalisation(*row.normalisation(), 255.0)
    if row.freeze_k is not None:
        model.freeze_prefix(row.freeze_k)
    out, xs = dict(loss=[], extra=[], logits=[]), []
    old = hip.set_deterministic(row.reductions == "deterministic")
    try:
        random.seed(row.seed)
        for p in range(row.passes):
            fed, _, y = row.batch(p)
            x = fed.to(device)
            if row.grads == "input":
                x.requires_grad_(True)
            xs.append(x)
            model.drop_path_sampler = row.drop_sampler(p)
            logits, extra = model(x, "train", None, init_first_layer=None, new_channel_init=None, cur_epoch=0)
            loss = torch.nn.functional.cross_entropy(logits, y.to(device)) + extra
            loss.backward()
            out["loss"].append(loss.item()); out["extra"].append(extra.item()); out["logits"].append(logits.detach().double().cpu())
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize(device)
        out["grads"] = {k: (None if p.grad is None else p.grad.detach().double().cpu()) for k, p in model.named_parameters()}
        out["requires_grad"] = {k: p.requires_grad for k, p in model.named_parameters()}
        out["xgrads"] = [x.grad.detach().double().cpu() for x in xs] if row.grads == "input" else None
        model.eval()
        if log is not None:
            log.append((EVAL_MARK, {}))
        with torch.no_grad():
            out["eval"] = model(row.batch(0)[0].to(device), "train", None).double().cpu()
    finally:
        hip.set_deterministic(old)
    out["seconds"] = time.perf_counter() - t0
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the comparator: the project's stated bounds (tests/test_model_gpu.py, tests/test_input_grad_gpu.py), nothing else
# ---------------------------------------------------------------------------------------------------------------------------------------------
LOGIT_BOUND, LOSS_BOUND, LOSS_BOUND_STOCHASTIC, EXTRA_REL, EXTRA_ABS = 3e-2, 5e-3, 1e-2, 2e-2, 1e-6
GRAD_REL, GRAD_COS, SMALL_REF, SMALL_GOT = 5e-2, 0.998, 1e-7, 1e-5
X_REL, X_COS = 5e-2, 0.998  # test_input_grad_gpu.py: REL_BOUND, COS_BOUND, per image and channel


def compare(row, ref, got):
    """(figures, failures): the distances of `got` (run_model) from `ref` (run_oracle) and one line per bound that is missed"""
    fail = []
    loss_bound = LOSS_BOUND_STOCHASTIC if row.copies == "stochastic" else LOSS_BOUND
    fig = dict(loss_err=0.0, logit_err=0.0, extra_err=0.0, worst_rel=(0.0, None), min_cos=(1.0, None), x_rel=None, x_cos=None)
    for p in range(row.passes):
        e = abs(got["loss"][p] - ref["loss"][p])
        fig["loss_err"] = max(fig["loss_err"], e)
        if not e <= loss_bound:
            fail.append(f"pass {p}: loss off by {e:.3e} (bound {loss_bound:g})")
        lg = ref["logits"][p]
        e = (got["logits"][p] - lg).abs().max().item() / lg.abs().max().item()
        fig["logit_err"] = max(fig["logit_err"], e)
        if not e <= LOGIT_BOUND:
            fail.append(f"pass {p}: logits off by {e:.3e} of max|ref| (bound {LOGIT_BOUND:g})")
        e, r = abs(got["extra"][p] - ref["extra"][p]), abs(ref["extra"][p])
        fig["extra_err"] = max(fig["extra_err"], e / r if r else e)
        if not e <= EXTRA_REL * r + EXTRA_ABS:
            fail.append(f"pass {p}: extra term {got['extra'][p]:.6e} against {ref['extra'][p]:.6e}")
    for name, g in got["grads"].items():
        r = ref["grads"][name]
        if not row.trains(name) or r is None:
            if g is not None:
                fail.append(f"{name}: a gradient where none is expected")
            if not row.trains(name) and got["requires_grad"][name]:
                fail.append(f"{name}: still trainable under freeze_prefix({row.freeze_k})")
            continue
        if g is None:
            fail.append(f"{name}: gradient missing")
            continue
        rn, gn = r.norm().item(), g.norm().item()
        if rn < SMALL_REF:
            if not gn < SMALL_GOT:
                fail.append(f"{name}: norm {gn:.3e} where the oracle's is {rn:.3e}")
            continue
        rel = (g - r).norm().item() / rn
        cos = (g * r).sum().item() / (gn * rn + 1e-30)
        if rel > fig["worst_rel"][0]:
            fig["worst_rel"] = (rel, name)
        if cos < fig["min_cos"][0]:
            fig["min_cos"] = (cos, name)
        if not (rel <= GRAD_REL and cos >= GRAD_COS):
            fail.append(f"{name}: rel L2 {rel:.3e}, cosine {cos:.6f}")
    if row.grads == "input":
        fig["x_rel"], fig["x_cos"] = 0.0, 1.0
        outside = [c for c in range(N_CHANNELS) if c not in row.picked]
        for p in range(row.passes):
            g, r = got["xgrads"][p], ref["xgrads"][p]
            if outside and g[:, outside].abs().max().item() != 0.0:
                fail.append(f"pass {p}: input gradient outside the channel subset is not exactly zero")
            for b, c in itertools.product(range(BATCH), row.picked):
                rn, gn = r[b, c].norm().item(), g[b, c].norm().item()
                if rn == 0.0:  # a channel whose tokens were all dropped and that no loss term reads: structurally zero on both sides
                    if gn != 0.0:
                        fail.append(f"pass {p}: input gradient of image {b} channel {c} is {gn:.3e} where the oracle's is exactly zero")
                    continue
                rel = (g[b, c] - r[b, c]).norm().item() / rn
                cos = (g[b, c] * r[b, c]).sum().item() / (gn * rn + 1e-300)
                fig["x_rel"], fig["x_cos"] = max(fig["x_rel"], rel), min(fig["x_cos"], cos)
                if not (rel <= X_REL and cos >= X_COS):
                    fail.append(f"pass {p}: input gradient of image {b} channel {c}: rel L2 {rel:.3e}, cosine {cos:.6f}")
    e = (got["eval"] - ref["eval"]).abs().max().item() / ref["eval"].abs().max().item()
    fig["eval_err"] = e
    if not e <= LOGIT_BOUND:
        fail.append(f"eval forward off by {e:.3e} of max|ref| (bound {LOGIT_BOUND:g})")
    return fig, fail


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the launch recorder: logs and forwards
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _public_wrappers(hip):
    for name in dir(hip):
        fn = getattr(hip, name)
        if callable(fn) and not name.startswith("_") and not isinstance(fn, type) and getattr(fn, "__module__", "") == hip.__name__:
            yield name, fn


def install_recorder(setattr_, post=None):
    """Wraps every public hip.* wrapper: the call is logged as (name, {argument name: scalar | "tensor" | None}) and forwarded.  post: optional
    {name: callable(arguments)} run after the real call (the injected defects of test_switch_pairs_gpu.py).  setattr_: monkeypatch.setattr.
    Returns the log."""
    from diverse_channel_vit_amd import hip
    log = []

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def wrapper(*a, **k):
            args = sig.bind(*a, **k)
            args.apply_defaults()
            log.append((name, {n: ("tensor" if torch.is_tensor(v) else v) for n, v in args.arguments.items()
                               if v is None or torch.is_tensor(v) or isinstance(v, (bool, int, float, str))}))
            res = fn(*a, **k)
            if post and name in post:
                post[name](args.arguments)
            return res
        return wrapper

    for name, fn in list(_public_wrappers(hip)):
        setattr_(hip, name, wrap(name, fn))
    return log


def check_launches(row, log):
    """Did the row's levels take effect?  `log`: the recorder's, of run_model(row, device, log).  What is said of the training step is read from
    the launches before EVAL_MARK alone, so the eval forward cannot meet it; the forward's own levels (pre-scaled q, the CLS-only query, the
    LayerNorm epilogue, the uint8 scale) are checked in the eval forward as well.  Returns the misses."""
    miss = []
    marks = [i for i, (n, _) in enumerate(log) if n == EVAL_MARK]
    if len(marks) != 1:
        return [f"{len(marks)} eval marks in the log: run_model was not given the recorder's log"]
    train, evl = log[:marks[0]], log[marks[0] + 1:]
    names = [n for n, _ in train]
    of = lambda n, part=train: [k for m, k in part if m == n]  # noqa: E731

    def iff(what, seen, expected):
        if bool(seen) != bool(expected):
            miss.append(f"{what}: {'seen' if seen else 'not seen'}, expected {'yes' if expected else 'no'}")

    iff("gemm_nt_resid_ln launched", "gemm_nt_resid_ln" in names, row.fuse_ln == "forced" and row.small)
    iff("gemm_nt_resid_ln launched in eval", of("gemm_nt_resid_ln", evl), row.fuse_ln == "forced" and row.small)
    fwd = of("attn_fwd") + of("attn_fwd", evl)
    per_fwd = [fwd[i:i + DEPTH] for i in range(0, len(fwd), DEPTH)]  # every forward (training passes, then eval) launches DEPTH of them
    if len(of("attn_fwd")) != DEPTH * row.passes or len(of("attn_fwd", evl)) != DEPTH:
        miss.append(f"{len(of('attn_fwd'))} + {len(of('attn_fwd', evl))} attn_fwd launches for {row.passes} training forwards and one eval forward "
                    f"of {DEPTH} blocks")
    iff("every attn_fwd prescaled", all(k["prescaled"] for k in fwd), row.prescaled)
    iff("no attn_fwd prescaled", not any(k["prescaled"] for k in fwd), not row.prescaled)
    iff("the last block's attn_fwd has nq == 1", all(f[-1]["nq"] == 1 for f in per_fwd), row.cls_tail)
    if any(k["nq"] is not None for f in per_fwd for k in f[:-1]) or (not row.cls_tail and any(f[-1]["nq"] is not None for f in per_fwd)):
        miss.append("an attn_fwd other than the CLS-only tail's is restricted to some query rows")
    iff("gemm_tn_acc_group launched", "gemm_tn_acc_group" in names, row.wgrad != "ungrouped_shared")
    iff("gather_tokens launched", "gather_tokens" in names, row.token_drop != "none")
    iff("some ln_bwd carries bf16_row_scale", any(k["bf16_row_scale"] is not None for k in of("ln_bwd")), row.drop_path > 0)
    if len(of("im2col")) != row.passes or len(of("im2col", evl)) != 1:
        miss.append(f"{len(of('im2col'))} + {len(of('im2col', evl))} im2col launches for {row.passes} training forwards and one eval forward")
    iff("every im2col carries scale", all(k["scale"] is not None for k in of("im2col") + of("im2col", evl)), row.input == "uint8")
    iff("no im2col carries scale", not any(k["scale"] is not None for k in of("im2col") + of("im2col", evl)), row.input != "uint8")
    iff("patch_dgrad launched", "patch_dgrad" in names, row.grads == "input")
    if len(of("attn_bwd")) != row.passes * row.backward_blocks():
        miss.append(f"{len(of('attn_bwd'))} attn_bwd launches, expected {row.passes} x {row.backward_blocks()}")
    iff("proxy_loss launched", "proxy_loss" in names, row.losses == "ortho_proxy_fused")
    iff("cast_bf16_sr launched", "cast_bf16_sr" in names, row.copies == "stochastic")
    return miss


def format_line(row, fig, seconds, tfig, tseconds):
    def four(f):
        return (f"loss {f['loss_err']:.2e} logits {f['logit_err']:.2e} grad rel {f['worst_rel'][0]:.2e} ({f['worst_rel'][1]}) "
                f"cos {f['min_cos'][0]:.6f} ({f['min_cos'][1]})")
    return f"{row.id} N={'/'.join(map(str, row.N))} {row.describe()} | {four(fig)} {seconds:.1f}s | twin: {four(tfig)} {tseconds:.1f}s"
