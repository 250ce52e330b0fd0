"""CPU tier of the fused BN(+add)+SiLU epilogue (``act="silu"``): reference
ops and modules against fp64 (silu_ref.py), the fuse pass, the argument
checks and pickling."""

import pickle

import pytest
import torch
import torch.nn as nn

import msbn
from msbn import ops
from msbn.nn import FrozenBatchNorm2d, SyncBatchNormAct2d, fuse_bn_act
from silu_ref import EPS, check_module, check_ops, draw, make_module

SHAPE = (3, 20, 7, 7)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_ops_vs_fp64(dtype, with_res, frozen):
    check_ops(draw(SHAPE, dtype), dtype, with_res, frozen=frozen)


@pytest.mark.parametrize("cls,training", [(SyncBatchNormAct2d, True),
                                          (SyncBatchNormAct2d, False),
                                          (FrozenBatchNorm2d, False)])
@pytest.mark.parametrize("with_res", [False, True])
def test_module_vs_fp64_autograd(with_res, cls, training):
    d = draw(SHAPE)
    check_module(make_module(cls, d, training), d, torch.float32, with_res)


def test_fuse_bn_act_folds_silu():
    for inplace in (False, True):
        seq = fuse_bn_act(nn.Sequential(nn.Sequential(
            nn.Conv2d(3, 8, 3), msbn.nn.BatchNorm2d(8), nn.SiLU(inplace=True),
            nn.Conv2d(8, 8, 1), FrozenBatchNorm2d(8), nn.SiLU(),
        )), inplace=inplace)[0]
        assert [type(m).__name__ for m in seq] == [
            "Conv2d", "SyncBatchNormAct2d", "Conv2d", "FrozenBatchNorm2d"]
        assert seq[1].act == "silu" and seq[1].relu and not seq[1].inplace
        assert seq[3].act == "silu" and seq[3].relu
        assert "act='silu'" in repr(seq[1]) and "act='silu'" in repr(seq[3])
    frozen = msbn.nn.freeze_batchnorm(seq)
    assert type(frozen[1]) is FrozenBatchNorm2d and frozen[1].act == "silu"


def test_silu_argument_checks():
    for kw in (dict(negative_slope=0.1), dict(inplace=True),
               dict(relu=False), dict(act="gelu")):
        with pytest.raises(ValueError):
            SyncBatchNormAct2d(4, **{"act": "silu", **kw})
    with pytest.raises(ValueError):
        FrozenBatchNorm2d(4, relu=True, negative_slope=0.1, act="silu")
    d = draw((2, 4, 3, 3))
    mean, invstd = ops.batch_norm_stats(d["x"], EPS)
    for relu, slope in ((True, 0.1), (False, 0.0)):
        with pytest.raises(ValueError):
            ops.batch_norm_elemt_act(d["x"], None, d["w"], d["b"], mean,
                                     invstd, relu, None, slope, act="silu")


@pytest.mark.parametrize("cls", [SyncBatchNormAct2d, FrozenBatchNorm2d])
def test_pickle_keeps_the_mode(cls):
    d = draw((2, 4, 3, 3))
    m = make_module(cls, d, False)
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.act == "silu" and torch.equal(m2(d["x"]), m(d["x"]))
    # a module pickled before the keyword existed has no such attribute
    del m2.__dict__["act"]
    old = pickle.loads(pickle.dumps(m2))
    want = cls(4, eps=EPS, relu=True)
    want.load_state_dict(m.state_dict())
    assert torch.equal(old(d["x"]), want.eval()(d["x"]))
    assert "act" not in repr(old)
