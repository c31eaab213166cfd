"""The bf16 operand copies of the encoder weights as one value.  Every GEMM of the encoder multiplies by a bf16 copy of the fp32 master weights
in the parameter arena; a forward takes a set of copies and its saved state keeps it, so its backward multiplies by the bits the forward used."""
import types

import torch

from . import hip

_BLOCKS_PER_DESC = 64  # workgroups dcv_cast_scaled_ranges spends on each descriptor


class _OperandCopies:
    """One set: `straight` (same offsets as the arena), `transposed` (the four Linear weights of every block, transposed in their slots: what
    the input-gradient GEMMs read; None in a forward-only set) and `qbias` [depth, 3 D] (the qkv bias, its q part pre-scaled when `prescaled`).
    `lay` is the read-only layout that every set of one arena shares: slot offsets, transpose and q descriptors, the q scale."""

    def __init__(self, lay, transposed=True):
        self.lay, self.prescaled = lay, False  # prescaled: set by refresh
        self.straight = torch.empty(lay.size, dtype=torch.bfloat16, device=lay.device)
        self.transposed = torch.empty_like(self.straight) if transposed else None
        self.qbias = torch.empty(lay.qbias_shape, dtype=torch.float32, device=lay.device)

    @classmethod
    def for_encoder(cls, slot, size, blocks, dim, q_scale, device):
        """The first set of an arena.  slot: {id(parameter): offset of its slot in floats}; size: the encoder's part of the arena in floats.
        Transpose descriptors {src offset, dst offset, rows, columns}: the four Linear weights of every block, in 64 x 64 tiles.  Pre-scaled q,
        two descriptors per block (hip.cast_scaled_ranges): the q rows of the qkv weight copy (kind 0, in place in the bf16 copy) and the qkv
        bias with its q part scaled (kind 1)."""
        mats = [w for b in blocks for w in (b.attn.qkv.weight, b.attn.proj.weight, b.mlp.fc1.weight, b.mlp.fc2.weight)]
        tdesc = [[slot[id(w)], slot[id(w)], *w.shape] for w in mats]
        qdesc = []
        for li, b in enumerate(blocks):
            ow, ob = slot[id(b.attn.qkv.weight)], slot[id(b.attn.qkv.bias)]
            qdesc += [[ow, ow, dim * dim, dim * dim, 0], [ob, li * 3 * dim, 3 * dim, dim, 1]]
        return cls(types.SimpleNamespace(slot=slot, size=size, device=device, q_scale=q_scale, qbias_shape=(len(blocks), 3 * dim),
                                         tdesc=torch.tensor(tdesc, dtype=torch.int64, device=device), tdesc_n=len(tdesc),
                                         tdesc_tiles=max([1] + [((w.shape[0] + 63) // 64) * ((w.shape[1] + 63) // 64) for w in mats]),
                                         qdesc=torch.tensor(qdesc, dtype=torch.int64, device=device)))

    def private(self, transposed):
        """A fresh, unfilled set on this set's layout (the descriptors are shared).  transposed=False: a forward-only set."""
        return _OperandCopies(self.lay, transposed)

    def w(self, p):
        """The straight copy of the weight p as a matrix: [p.shape[0], everything else]."""
        o = self.lay.slot[id(p)]
        return self.straight[o:o + p.numel()].view(p.shape[0], p.numel() // p.shape[0])

    def wt(self, p):
        """The transposed copy of the matrix p."""
        o = self.lay.slot[id(p)]
        return self.transposed[o:o + p.numel()].view(p.numel() // p.shape[0], p.shape[0])

    def refresh(self, arena, *, prescale_q, seed=None):
        """Fills the set from the arena: round-to-nearest, or stochastically rounded with the device int32 word `seed` (the caller bumps it).
        prescale_q: the W_q rows of the straight copy and the q part of the bias copy times the q scale; the transposed copy stays unscaled
        (the input-gradient GEMM multiplies by it the gradient with respect to the unscaled q)."""
        lay, sr = self.lay, () if seed is None else (seed,)
        cast, cast_t = (hip.cast_bf16, hip.cast_transpose_bf16) if seed is None else (hip.cast_bf16_sr, hip.cast_transpose_bf16_sr)
        cast(arena, self.straight, lay.size, *sr)
        if self.transposed is not None:
            cast_t(arena, self.transposed, lay.tdesc, lay.tdesc_n, lay.tdesc_tiles, *sr)
        if prescale_q:
            hip.cast_scaled_ranges(arena, self.straight, self.qbias, lay.qdesc, lay.qdesc.shape[0], _BLOCKS_PER_DESC, lay.q_scale, *sr)
        self.prescaled = bool(prescale_q)
