"""The train step against the fp64 oracle over all pairs of its switches (tests/switch_pairs.py: the factor table, the frozen covering array, the
runners).  Every row runs its training passes and one eval forward on the HIP path, under a pass-through recorder of the hip.* wrappers that
proves the row's levels took effect, and is held to the project's stated bounds (test_model_gpu.py, test_input_grad_gpu.py; no new numbers).

When a row misses a bound its plain twin — the same row with pre-scaled q, the LayerNorm epilogue, the CLS tail, grouping, the second stream,
atomics and stochastic copies all off — is run and reported beside it.  Twin inside the bounds: the combination is wrong, the cause is in the product.
Twin outside as well: the row's inputs are too small for the bound (few tokens); that level's inputs are changed, never a bound.

Pair coverage promises every PAIR of levels once, not triples.  Needs an MI355X (-m gpu)."""
import pytest

import switch_pairs as sp

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(row):
    """a row's fp64 reference, computed once (the twin shares it: the twin's levels change nothing the oracle reads)"""
    if row.index not in _ORACLE:
        _ORACLE[row.index] = sp.run_oracle(row)
    return _ORACLE[row.index]


def _figures(tag, fig):
    x = "" if fig["x_rel"] is None else f", input grad rel {fig['x_rel']:.2e} cos {fig['x_cos']:.6f}"
    return (f"{tag}: loss {fig['loss_err']:.2e}, logits {fig['logit_err']:.2e}, extra {fig['extra_err']:.2e}, eval {fig['eval_err']:.2e}, grad rel "
            f"{fig['worst_rel'][0]:.2e} ({fig['worst_rel'][1]}), cos {fig['min_cos'][0]:.6f} ({fig['min_cos'][1]}){x}")


@pytest.mark.parametrize("row", sp.rows(), ids=lambda r: r.id)
def test_row_against_the_oracle(gpu_device, monkeypatch, row):
    log = sp.install_recorder(monkeypatch.setattr)
    got = sp.run_model(row, gpu_device, log)
    missed = sp.check_launches(row, log)
    fig, fail = sp.compare(row, _oracle(row), got)
    print(f"{row.id} N={row.N} {row.describe()}")
    print(_figures(row.id, fig))
    if fail:  # adjudication: the plain twin on the same inputs
        twin = row.plain_twin()
        tfig, tfail = sp.compare(twin, _oracle(row), sp.run_model(twin, gpu_device))
        print(_figures(twin.id, tfig))
        verdict = "the twin misses too: inputs too small for the bound" if tfail else "the twin passes: the COMBINATION is wrong"
        fail = fail + [verdict] + [f"twin: {t}" for t in tfail]
    assert not missed, missed
    assert not fail, "\n".join(fail)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# would the sweep notice?  Three defects that each need two levels at once, injected into the python wrappers' results
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _defect_droppath_x_tokendrop(row):
    """the residual epilogues mishandle the DropPath factor when the rows per sample are not the undropped token count"""
    def resid(a):
        if a["aux2"] is not None and a["epilogue"] == _hip().EPI_BIAS_RESID_F32 and a["T"] not in (0, 1, row.N_full):
            a["out"][:, ::2].mul_(1.5)

    def resid_ln(a):
        if a["branch_scale"] is not None and a["T"] not in (0, 1, row.N_full):
            a["x_out"][:, ::2].mul_(1.5)
    return dict(gemm_nt=resid, gemm_nt_resid_ln=resid_ln)


def _defect_tail_x_prescaled(row):
    """the CLS-only query path of the pre-scaled attention forward returns a scaled output"""
    def fwd(a):
        if a["nq"] == 1 and a["prescaled"]:
            a["o"].view(a["B"], a["N"], -1)[:, 0].mul_(1.5)
    return dict(attn_fwd=fwd)


def _defect_group_x_atomic(row):
    """the grouped weight-gradient launch's first product is wrong in the atomic mode"""
    def group(a):
        if not _hip().is_deterministic():
            a["items"][0][2].mul_(2.0)
    return dict(gemm_tn_acc_group=group)


def _hip():
    from diverse_channel_vit_amd import hip
    return hip


# name -> (the defect, does the row hold the first level, does it hold the second)
DEFECTS = {
    "droppath_x_tokendrop": (_defect_droppath_x_tokendrop, lambda r: r.drop_path > 0, lambda r: r.token_drop != "none"),
    "tail_x_prescaled": (_defect_tail_x_prescaled, lambda r: r.cls_tail, lambda r: r.prescaled),
    "group_x_atomic": (_defect_group_x_atomic, lambda r: r.wgrad != "ungrouped_shared", lambda r: r.reductions == "atomic"),
}
WIDE = 4.0  # a flagged row has to miss some bound by at least this factor


def _miss_factor(row, fig):
    """the largest ratio of a figure to its bound (gradient cosine: of the distances from 1)"""
    loss_bound = sp.LOSS_BOUND_STOCHASTIC if row.copies == "stochastic" else sp.LOSS_BOUND
    return max(fig["loss_err"] / loss_bound, fig["logit_err"] / sp.LOGIT_BOUND, fig["eval_err"] / sp.LOGIT_BOUND,
               fig["worst_rel"][0] / sp.GRAD_REL, (1.0 - fig["min_cos"][0]) / (1.0 - sp.GRAD_COS))


@pytest.mark.parametrize("name", list(DEFECTS))
def test_the_sweep_flags_pair_defects(gpu_device, monkeypatch, name):
    """Each defect fires only where two levels meet.  Every row that holds the pair must fail the comparator, by a wide factor.  Two one-level
    rows per defect (not per flagged row) run with the defect installed and must pass: the first row of the table that holds only the first
    level, and the first that holds only the second.  The defect's condition cannot be met in either, so what they show is that the injection
    itself, installed and consulted on every launch, disturbs nothing.  Measured on the MI355X (smallest miss factor
    over the flagged rows): droppath_x_tokendrop 396x (logits), tail_x_prescaled 9.6x (gradient cosine), group_x_atomic 20x (the doubled gradient:
    relative error 1.0 against 5e-2)."""
    make, first, second = DEFECTS[name]
    rows = sp.rows()
    both = [r for r in rows if first(r) and second(r)]
    only = [next(r for r in rows if first(r) and not second(r)), next(r for r in rows if second(r) and not first(r))]
    assert both, "no row holds the pair"
    for row in both + only:
        with monkeypatch.context() as m:
            sp.install_recorder(m.setattr, post=make(row))
            got = sp.run_model(row, gpu_device)
        fig, fail = sp.compare(row, _oracle(row), got)
        if row in both:
            factor = _miss_factor(row, fig)
            print(f"{name}: {row.id} flagged, misses a bound by {factor:.1f}x ({len(fail)} lines)")
            assert fail, f"{name}: {row.id} holds the pair and passes"
            assert factor >= WIDE, (name, row.id, factor)
        else:
            print(f"{name}: {row.id} holds one level only and passes")
            assert not fail, f"{name}: {row.id} holds one level only and fails:\n" + "\n".join(fail)
