"""Host side of weight averaging (no GPU): dcv_avg_update is exported and refuses every documented bad argument before any HIP call;
AveragedModel wraps a CPU model without touching the GPU, has the state-dict layout of torch.optim.swa_utils.AveragedModel (each loads
the other's), refuses to average on the CPU, and torch's update_bn leaves the loader alone (the model has no BatchNorm)."""
import ctypes as C
import math

import pytest
import torch
from torch.optim import swa_utils

from conftest import load_golden


class Cfg(dict):
    """A DictConfig stand-in that copy.deepcopy can take apart (dunder lookups are not keys)."""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return self.get(k)


def tiny(**over):
    import diverse_channel_vit_amd as dcv
    meta, _ = load_golden("tiny_e2e")
    cfg = Cfg(meta["cfg"], in_channel_names=[f"c{i}" for i in range(meta["n_channels"])], img_size=[meta["img"]],
              num_classes=over.get("num_classes", meta["num_classes"]))
    model = dcv.dichavit(cfg, mapper={k: list(v) for k, v in meta["mapper"].items()})
    assert len(model.feature_extractor.blocks) == 12
    return model


def test_avg_update_is_exported():
    from diverse_channel_vit_amd import hip
    assert "dcv_avg_update" in hip.EXPORTS
    assert hasattr(hip.load(), "dcv_avg_update") and callable(hip.avg_update)
    assert (hip.AVG_SWA, hip.AVG_EMA) == (0, 1)


def test_avg_update_error_codes():
    """Every refusal of include/dcv.h, with dummy non-null aligned addresses: each call carries one bad argument, so none reaches a launch
    (a launch on this machine would fail with DCV_ERR_LAUNCH = -4, or fault on the dummy addresses: neither code is accepted here)."""
    from diverse_channel_vit_amd import hip
    lib = hip.load()
    OK, SHAPE, ALIGN, UNSUPPORTED, NULL = 0, -1, -2, -3, -5
    A, P, W = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    ok = [A, P, 64, hip.AVG_SWA, 0.0, 0, None, 0, None]

    def call(**kw):
        a = list(ok)
        for i, val in kw.items():
            a[int(i[1:])] = val
        return lib.dcv_avg_update(*a)

    assert call(a0=None) == NULL and call(a1=None) == NULL
    assert call(a2=-1) == SHAPE and call(a2=-(1 << 40)) == SHAPE
    for i in (0, 1):
        for off in (4, 8, 12):
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == ALIGN, (i, off)
    assert call(a6=C.c_void_p(0x3004)) == ALIGN  # the count is an int64 word
    for bad in (-1, 2, 77):
        assert call(a3=bad) == UNSUPPORTED, bad
    for bad in (-1e-6, 1.0000001, -1.0, 2.0, math.nan, math.inf, -math.inf):
        assert call(a3=hip.AVG_EMA, a4=bad) == SHAPE, bad
    assert call(a5=-1) == SHAPE and call(a3=hip.AVG_EMA, a4=0.5, a5=-7) == SHAPE
    assert call(a7=-1) == SHAPE
    # the documented order: a null pointer before a bad n, a bad n before alignment, alignment before the mode, the mode before the weight
    assert call(a0=None, a2=-1) == NULL
    assert call(a2=-1, a0=C.c_void_p(0x1004)) == SHAPE
    assert call(a0=C.c_void_p(0x1004), a3=9) == ALIGN
    assert call(a3=9, a4=math.nan) == UNSUPPORTED
    # n == 0 succeeds and launches nothing, in both modes, with the count by value or in a (never read) device word
    assert call(a2=0) == OK and call(a2=0, a3=hip.AVG_EMA, a4=1.0) == OK and call(a2=0, a6=W, a5=-1, a7=3) == OK


def test_cpu_construction_and_state_dict_layout():
    import diverse_channel_vit_amd as dcv
    m = tiny()
    m.eval()
    ours, theirs = dcv.AveragedModel(m), swa_utils.AveragedModel(m)
    assert isinstance(ours, torch.nn.Module) and ours.module is not m and not ours.module.training
    assert ours.n_averaged.dtype == torch.long and ours.n_averaged.device.type == "cpu" and int(ours.n_averaged) == 0
    assert ours.module._dp is None and ours.module._arena is None
    assert ours.module.feature_extractor._owner() is ours.module  # the copy's encoder runs on the copy's weights
    sd_o, sd_t = ours.state_dict(), theirs.state_dict()
    assert set(sd_o) == set(sd_t) and list(sd_o)[0] == list(sd_t)[0] == "n_averaged"
    assert all(sd_o[k].shape == sd_t[k].shape and sd_o[k].dtype == sd_t[k].dtype for k in sd_o)
    for p, q in zip(ours.module.parameters(), m.parameters()):
        assert p is not q and p.data_ptr() != q.data_ptr() and torch.equal(p, q)
    # both directions, with values that tell the two apart
    with torch.no_grad():
        for p in theirs.module.parameters():
            p.add_(1.0)
        theirs.n_averaged.fill_(7)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    assert int(ours.n_averaged) == 7
    assert all(torch.equal(p, q) for p, q in zip(ours.module.parameters(), theirs.module.parameters()))
    with torch.no_grad():
        for p in ours.module.parameters():
            p.mul_(0.5)
        ours.n_averaged.fill_(3)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    assert int(theirs.n_averaged) == 3
    assert all(torch.equal(p, q) for p, q in zip(ours.module.parameters(), theirs.module.parameters()))
    for kw in (dict(avg="median"), dict(avg="ema", decay=1.5), dict(avg="ema", decay=-0.1)):
        with pytest.raises(ValueError):
            dcv.AveragedModel(m, **kw)
    assert dcv.AveragedModel(m.train()).module.training  # the copy keeps the model's mode, as torch's does


def test_no_cpu_fallback():
    import diverse_channel_vit_amd as dcv
    m = tiny()
    for kind in ("swa", "ema"):
        a = dcv.AveragedModel(m, avg=kind)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            a.update_parameters(m)
        assert int(a.n_averaged) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dcv.AveragedModel(m)(torch.zeros(2, 3, 32, 32), "train", None)  # forward is the copy's forward


def test_update_bn_returns_without_touching_the_loader():
    import diverse_channel_vit_amd as dcv

    class Loader:
        def __iter__(self):
            raise AssertionError("update_bn iterated the loader: the model has no BatchNorm")

    a = dcv.AveragedModel(tiny())
    assert swa_utils.update_bn(Loader(), a) is None


def test_defaults_leave_the_step_and_the_checkpoint_alone(tmp_path):
    """GraphedTrainStep / save_checkpoint / load_checkpoint take the new keyword arguments and, at their defaults, write the keys they
    wrote before (no averaged_params) and read files without it."""
    import inspect
    import diverse_channel_vit_amd as dcv
    assert inspect.signature(dcv.GraphedTrainStep.__init__).parameters["averager"].default is None
    assert inspect.signature(dcv.save_checkpoint).parameters["averaged"].default is None
    assert inspect.signature(dcv.load_checkpoint).parameters["averaged"].default is None
    m = tiny()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    plain, with_avg = str(tmp_path / "plain.pt"), str(tmp_path / "avg.pt")
    dcv.save_checkpoint(plain, m, opt, epoch=3)
    a = dcv.AveragedModel(m, avg="ema", decay=0.9)
    with torch.no_grad():
        a.n_averaged.fill_(11)
        a.module.proxies.add_(2.0)
    dcv.save_checkpoint(with_avg, m, opt, epoch=4, averaged=a)
    keys = set(torch.load(plain, weights_only=True))
    assert "averaged_params" not in keys and set(torch.load(with_avg, weights_only=True)) == keys | {"averaged_params"}
    assert dcv.load_checkpoint(with_avg, tiny()) == 4  # read without it: the key is ignored
    b = dcv.AveragedModel(tiny())
    assert dcv.load_checkpoint(with_avg, tiny(), averaged=b) == 4
    assert int(b.n_averaged) == 11 and torch.equal(b.module.proxies, a.module.proxies)
    with pytest.raises(ValueError, match="averaged_params"):
        dcv.load_checkpoint(plain, tiny(), averaged=b)
