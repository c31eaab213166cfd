"""The bf16 operand copies as a value (diverse_channel_vit_amd/operands.py: _OperandCopies) without a GPU.  Every hip.* wrapper is replaced by a
recorder and the model of test_launch_sequence_cpu runs on CPU tensors (4 blocks, D = 192, 3 channels, 32 x 32, patch 8: B = 2, N = 49).

Launch sequences: tests/golden/operand_copies_launches.json holds, per scenario, the launch names and a SHA-256 over every launch's name,
argument shapes, dtypes, strides and keyword arguments, recorded on the commit before the copies became a value
(tests/golden/make_operand_copies_launches.py).  The scenarios replayed here must give the same record.

Provenance: the recorder also keeps the storage address of every tensor argument, so a test can say which buffer a launch read or wrote: a
training step multiplies by the model's own set, an inspection call touches none of the model's three buffers."""
import contextlib
import hashlib
import json
import os

import pytest
import torch

import diverse_channel_vit_amd as dcv
from diverse_channel_vit_amd import hip
from test_launch_sequence_cpu import DEPTH, _model, _sig, dichavit

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "operand_copies_launches.json")


def _ptrs(v):
    """The storage addresses of the tensors in v, which may nest lists, tuples and dicts."""
    if torch.is_tensor(v):
        return (v.untyped_storage().data_ptr(),)
    if isinstance(v, dict):
        v = list(v.values())
    return tuple(q for e in v for q in _ptrs(e)) if isinstance(v, (list, tuple)) else ()


@contextlib.contextmanager
def recording():
    """test_launch_sequence_cpu's recorder as a context (the golden's script uses it outside pytest), with the addresses: a log entry is
    (name, signature of the positional arguments, of the keyword arguments, addresses per positional argument, addresses of the keywords)."""
    log, saved = [], {}
    for name in dir(hip):
        fn = getattr(hip, name)
        if callable(fn) and not name.startswith("_") and not isinstance(fn, type) and getattr(fn, "__module__", "") == hip.__name__:
            saved[name] = fn
            setattr(hip, name, lambda *a, _n=name, **k: log.append((_n, _sig(a), _sig(k), tuple(_ptrs(e) for e in a), _ptrs(k))))
    saved_check, saved_size = dichavit.DiChaViT.__dict__["_check_input"], dichavit._SIZES.get("tiny")
    dichavit.DiChaViT._check_input = staticmethod(lambda x: None)
    dichavit._SIZES["tiny"] = (192, DEPTH, 3)
    try:
        yield log
    finally:
        for name, fn in saved.items():
            setattr(hip, name, fn)
        dichavit.DiChaViT._check_input = saved_check
        if saved_size is None:
            del dichavit._SIZES["tiny"]
        else:
            dichavit._SIZES["tiny"] = saved_size


@pytest.fixture
def log():
    with recording() as entries:
        yield entries


def _take(log):
    out = list(log)
    del log[:]
    return out


def summary(entries):
    """What the golden keeps of a recorded scenario: names, and one hash over names, shapes, dtypes, strides and keyword arguments."""
    canon = json.dumps([[n, a, k] for n, a, k, _, _ in entries], sort_keys=True, default=str)
    return {"names": [e[0] for e in entries], "sha256": hashlib.sha256(canon.encode()).hexdigest()}


# ---- scenarios ---------------------------------------------------------------------------------------------------------------------------------
def _images(px=32):
    return torch.zeros(2, 3, px, px)


def _train_model(tail=True, prescaled=True):
    model = _model().train()
    model.cls_only_tail, model.attn_prescaled, model.stochastic_weight_rounding = tail, prescaled, True
    return model


def _forward(model, x):
    out, extra = model(x, "train")
    return out.sum() + extra


def _step(model, x):
    _forward(model, x).backward()


def _views_step(model):
    feats, extra = model.forward_views([_images(32), _images(16)], "train")
    (feats.sum() + extra).backward()


INSPECTIONS = {
    "get_last_selfattention": lambda m, x: m.feature_extractor.get_last_selfattention(x, chunk="train", layer_idx=2),
    "get_intermediate_layers": lambda m, x: m.feature_extractor.get_intermediate_layers(x, n=[1, 3], chunk="train", pool="channel"),
    "get_channel_attention": lambda m, x: m.feature_extractor.get_channel_attention(x, n=[1, 3], chunk="train", queries="channel"),
    "get_attention_rollout": lambda m, x: m.feature_extractor.get_attention_rollout(x, chunk="train", start_layer=1),
    "get_attention_relevance start_layer=0": lambda m, x: m.get_attention_relevance(x, torch.zeros(2, dtype=torch.long), chunk="train", start_layer=0),
    "get_attention_relevance start_layer=2": lambda m, x: m.get_attention_relevance(x, torch.zeros(2, dtype=torch.long), chunk="train", start_layer=2),
}
FORWARD_ONLY = [k for k in INSPECTIONS if "relevance" not in k]


def _inspected_step(call):
    """A training forward, the inspection call, then the forward's backward: all three are recorded."""
    model, x = _train_model(), _images()
    loss = _forward(model, x)
    call(model, x)
    loss.backward()


SCENARIOS = {
    **{f"train step tail={int(t)} prescaled={int(p)}": (lambda t=t, p=p: _step(_train_model(t, p), _images())) for t in (False, True) for p in (False, True)},
    "train step, x requires grad": lambda: _step(_train_model(), _images().requires_grad_()),
    "train step, freeze_prefix(2)": lambda: _step(_train_model().freeze_prefix(2), _images()),
    "forward_views 32 px + 16 px": lambda: _views_step(_train_model()),
    **{f"{name} inside a train step": (lambda c=call: _inspected_step(c)) for name, call in INSPECTIONS.items()},
}


def record_all():
    out = {}
    for name, run in SCENARIOS.items():
        with recording() as entries:
            run()
            out[name] = summary(entries)
    return out


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_launch_sequence_is_the_recorded_one(log, name):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert set(want) == set(SCENARIOS)
    SCENARIOS[name]()
    got = summary(log)
    assert got["names"] == want[name]["names"]
    assert got["sha256"] == want[name]["sha256"]


# ---- provenance --------------------------------------------------------------------------------------------------------------------------------
def _addr(t):
    return t.untyped_storage().data_ptr()


def _weights_of(entries):
    """The address of the weight operand (second positional argument) of every gemm_nt launch."""
    return [e[3][1][0] for e in entries if e[0] == "gemm_nt"]


def test_a_training_step_multiplies_by_the_models_own_set(log):
    model, x = _train_model(), _images().requires_grad_()
    loss = _forward(model, x)
    fwd = _take(log)
    ops = model._ops
    straight, transposed = _addr(ops.straight), _addr(ops.transposed)
    assert len({straight, transposed, _addr(ops.qbias)}) == 3
    assert _weights_of(fwd) == [straight] * (1 + 4 * DEPTH)  # the patch projection and four linear layers per block
    assert [e[0] for e in fwd[:3]] == ["cast_bf16_sr", "cast_transpose_bf16_sr", "cast_scaled_ranges"]
    assert [e[3][1][0] for e in fwd[:2]] == [straight, transposed] and fwd[2][3][1:3] == ((straight,), (_addr(ops.qbias),))
    loss.backward()
    bwd = _take(log)
    assert _weights_of(bwd) == [transposed] * 16  # four input-gradient GEMMs per block, the CLS-only tail included
    dgrad = [e for e in bwd if e[0] == "patch_dgrad"]
    assert len(dgrad) == 1 and dgrad[0][3][1] == (straight,)  # the projection copy the forward multiplied by
    assert not any(e[0].startswith("cast_") and e[3][1][0] in (straight, transposed) for e in bwd)


@pytest.mark.parametrize("name", list(INSPECTIONS))
def test_an_inspection_call_leaves_the_models_set_alone(log, name):
    model, x = _train_model(), _images()
    loss = _forward(model, x)
    ops = model._ops
    own = {_addr(ops.straight), _addr(ops.transposed), _addr(ops.qbias)}
    seed = model._sr_seed.clone()
    _take(log)
    INSPECTIONS[name](model, x)
    call = _take(log)
    assert call and not any(own & set(q for arg in e[3] for q in arg) or own & set(e[4]) for e in call)  # neither read nor written
    assert torch.equal(model._sr_seed, seed) and model._ops is ops
    names = [e[0] for e in call]
    assert names[0] == "cast_bf16" and "cast_bf16_sr" not in names
    assert ("cast_transpose_bf16" in names) == (name not in FORWARD_ONLY)
    if name not in FORWARD_ONLY:  # the call's own backward multiplies by its private transposed copy
        private = call[names.index("cast_transpose_bf16")][3][1][0]
        assert set(_weights_of(call)[-4:]) == {private}
    loss.backward()
    bwd = _take(log)
    assert _weights_of(bwd) == [_addr(ops.transposed)] * 16


def test_a_forward_only_private_set_has_no_transposed_buffer(log):
    model, x = _train_model(), _images()
    with torch.no_grad():
        model(x, "train")
    ops = model._ops
    _take(log)
    private = ops.private(transposed=False)
    assert private.transposed is None and private.straight.shape == ops.straight.shape and private.qbias.shape == ops.qbias.shape
    assert not log  # a fresh set is unfilled: nothing is launched
    w = model.feature_extractor.blocks[1].attn.qkv.weight
    private.refresh(model._arena, prescale_q=True)
    assert [e[0] for e in _take(log)] == ["cast_bf16", "cast_scaled_ranges"] and private.prescaled
    assert private.w(w).shape == w.shape and _addr(private.w(w)) == _addr(private.straight) != _addr(ops.straight)
    assert private.w(w).data_ptr() - private.straight.data_ptr() == ops.w(w).data_ptr() - ops.straight.data_ptr()  # one layout
    assert ops.wt(w).shape == w.t().shape and ops.wt(w).is_contiguous()
    both = ops.private(transposed=True)
    both.refresh(model._arena, prescale_q=False)
    assert [e[0] for e in _take(log)] == ["cast_bf16", "cast_transpose_bf16"] and not both.prescaled


def test_averaged_model_leaves_the_operand_copies_out(log, monkeypatch):
    import test_launch_sequence_cpu
    from test_weight_average_cpu import Cfg
    monkeypatch.setattr(test_launch_sequence_cpu, "Cfg", Cfg)  # a configuration that copy.deepcopy can take apart
    model = _train_model()
    with torch.no_grad():
        model(_images(), "train")
    assert model._ops is not None
    avg = dcv.AveragedModel(model)
    assert avg.module._ops is None and avg.module._arena is None
    assert model._ops is not None
