"""The switch sweep's table and inputs, checked without a GPU: the frozen rows are the generator's, cover every allowed pair and respect the
constraints; the shapes reach every token-count class; the pinned draws have the properties the sweep relies on; a constructed model has every
attribute the rows set; and the fp64 oracle alone runs every row to finite losses and non-zero gradients — the inputs are sound before any
GPU bound is blamed."""
import itertools
import math

import pytest
import torch

import switch_pairs as sp


def test_frozen_rows_are_the_generators_and_cover_every_allowed_pair():
    assert list(sp.ROWS) == sp.generate(), "the frozen table is not what the generator produces"
    assert len(sp.ROWS) <= sp.MAX_ROWS
    need = sp.allowed_pairs()
    have = set().union(*(sp.pairs_of(r) for r in sp.ROWS))
    assert need <= have, sorted(need - have)
    # the allowed pairs are all pairs but the ones a constraint names: every constraint is a predicate over two factors
    every = {(i, li, j, lj) for i, j in itertools.combinations(range(len(sp.NAMES)), 2)
             for li in range(len(sp.FACTORS[i][1])) for lj in range(len(sp.FACTORS[j][1]))}
    barred = {p for p in every if not sp.allowed({sp.NAMES[p[0]]: sp.FACTORS[p[0]][1][p[1]], sp.NAMES[p[2]]: sp.FACTORS[p[2]][1][p[3]]})}
    assert need == every - barred and len(barred) == 2 + 1 + 2 + 1 + 2
    assert not have & barred


def test_rows_respect_the_constraints_and_so_do_their_twins():
    assert len(sp.FACTORS) == 15 and all(len(lv) <= 4 for _, lv in sp.FACTORS)
    for row in sp.rows():
        for r in (row, row.plain_twin()):
            d = dict(zip(sp.NAMES, r.levels))
            assert all(d[f] in sp.LEVELS[f] for f in sp.NAMES)
            assert [t for t, pred in sp.EXCLUDES if pred(d)] == [], r.id
        t = row.plain_twin()
        assert all(getattr(t, f) == v for f, v in sp.PLAIN.items()) and t.losses != "ortho_proxy_fused"
        assert (t.seed, t.keeps, t.N) == (row.seed, row.keeps, row.N)  # the same inputs and draws
        assert [getattr(t, f) for f in sp.NAMES[:9] if f != "losses"] == [getattr(row, f) for f in sp.NAMES[:9] if f != "losses"]


def test_token_counts_reach_both_sides_of_the_attention_tiles():
    seen = sorted({n for row in sp.rows() for n in row.N})
    assert any(n < 64 for n in seen) and any(64 <= n <= 128 for n in seen) and any(n > 128 for n in seen), seen
    assert sp.BATCH >= 3


def test_pinned_draws():
    for row in sp.rows():
        for p in range(row.passes):
            keep = row.keeps[p]
            if row.token_drop == "none":
                assert keep is None
            else:
                assert keep[0] == 0 and sorted(set(keep)) == keep and 3 <= len(keep) < row.N_full and keep[-1] < row.N_full, row.id
            masks = row.drop_masks(p)
            if row.drop_path == 0:
                assert masks is None and row.drop_sampler(p) is None
                continue
            m = torch.stack(masks)  # [2 (DEPTH - 1), B]: block 1 attention, block 1 MLP, ...
            assert m.shape == (2 * (sp.DEPTH - 1), sp.BATCH) and set(m.unique().tolist()) <= {0.0, 1.0}
            assert (m[-2] == 0).any(), "no sample dropped in the last block's attention branch"
            assert (m.min(dim=0).values == 1).any(), "no sample kept everywhere"
            assert (m.max(dim=1).values == 1).all(), "a branch drops the whole batch"
            s = row.drop_sampler(p)
            for bi, (j, br) in itertools.product(range(1, sp.DEPTH), enumerate(("attn", "mlp"))):
                assert torch.equal(s(bi, br, sp.BATCH, None).double(), masks[2 * (bi - 1) + j])
    assert len({r.freeze_k for r in sp.rows()}) == 3  # None, a prefix that ends below the last block, and one that ends at it


def test_every_rows_levels_can_take_effect_in_its_backward():
    """The recorder asserts `gemm_tn_acc_group launched` exactly on the rows with a grouped level, with no exception: so every such row needs
    a block below the CLS-only tail in its backward (the tail launches its products one by one), whatever freeze_prefix leaves of it."""
    rows = sp.rows()
    for row in rows:
        assert row.backward_blocks() >= 1 and (row.freeze_k is None or 0 < row.freeze_k < sp.DEPTH), row.id
        assert row.plain_twin().freeze_k == row.freeze_k, row.id
        if row.wgrad != "ungrouped_shared":
            assert row.small and row.grouped_blocks() >= 1, f"{row.id}: no block of its backward takes the grouped launch"
    # the frozen prefix still meets the CLS tail right under it (block 11 alone, as the tail), and ends at the last block without the tail
    assert any(r.freeze_k == sp.DEPTH - 1 and r.cls_tail for r in rows) and any(r.freeze_k == sp.DEPTH - 1 and not r.cls_tail for r in rows)
    assert any(r.freeze_k == sp.DEPTH // 2 and r.cls_tail for r in rows)


def test_a_constructed_model_has_every_switch_with_its_documented_default(monkeypatch):
    for v in sp.SWITCH_ENV:
        monkeypatch.delenv(v, raising=False)
    for row in sp.rows()[:2]:
        model = sp.new_model(row)
        for attr, default in sp.SWITCH_DEFAULTS.items():
            assert hasattr(model, attr), attr
            assert getattr(model, attr) == default, (attr, getattr(model, attr))
        assert len(model.feature_extractor.blocks) == sp.DEPTH
        rates = model.feature_extractor.drop_path_rates
        assert rates[0] == 0.0 and abs(rates[-1] - row.drop_path) < 1e-6
        assert hasattr(model, "freeze_prefix") and hasattr(model, "set_input_normalisation")
        sp.set_switches(model, row)
        assert model.hcs_sampler(model, "train", list(range(sp.N_CHANNELS))) == (row.picked, row.picked)
        names = {k for k, _ in model.named_parameters()}
        assert names == set(sp.state(row, torch.float32)), names ^ set(sp.state(row, torch.float32))
        if row.freeze_k is None:
            r1 = sp.Row(0, row.levels[:7] + ("freeze_prefix",) + row.levels[8:])
            model.freeze_prefix(r1.freeze_k)
            assert 0 < r1.freeze_k < sp.DEPTH - 1 and all(p.requires_grad == r1.trains(k) for k, p in model.named_parameters())


@pytest.mark.parametrize("row", sp.rows(), ids=lambda r: r.id)
def test_the_oracle_runs_the_row(row):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    ref = sp.run_oracle(row)
    assert len(ref["loss"]) == row.passes and all(math.isfinite(v) for v in ref["loss"] + ref["extra"])
    assert all(torch.isfinite(lg).all() and lg.shape == (sp.BATCH, sp.NUM_CLASSES) for lg in ref["logits"])
    assert all((e != 0) == (row.losses != "none") for e in ref["extra"])  # the ortho term is a mean of cosines: either sign
    assert torch.isfinite(ref["eval"]).all() and ref["eval"].shape == (sp.BATCH, sp.NUM_CLASSES)
    for name, g in ref["grads"].items():
        if not row.trains(name):
            assert g is None, name
        elif name == "proxies":
            assert g is None  # the class proxies belong to the CHAMMI loss: the regular train step does not read them
        elif name.endswith("channel_emb_proxies") and row.channels == 1:
            assert g.norm().item() == 0.0  # one channel: the proxy term is the cross-entropy of a single class, identically zero
        else:
            assert g is not None and torch.isfinite(g).all() and g.norm().item() > 0, name
    if row.grads == "input":
        outside = [c for c in range(sp.N_CHANNELS) if c not in row.picked]
        for g in ref["xgrads"]:
            assert torch.isfinite(g).all() and g[:, row.picked].norm().item() > 0 and not g[:, outside].any()
    else:
        assert ref["xgrads"] is None
