"""The pose model hosts, host side (no GPU): which class carries what (pose/host.py, pose/exact.py, one module per family), the
drop-in surface of pose.models, the (label, dtype, device) memo of HipModule, and reproducible construction."""
import functools

import pytest
import torch

from flowtrack.pytorch_amd.engine import HipModule
from flowtrack.pytorch_amd.pose import models
from flowtrack.pytorch_amd.pose.host import PoseHost

RESNET_ONLY = ("fuse_stage_exit", "fuse_bottleneck", "fuse_shortcut", "split_lanes", "split_lanes4", "cluster_kernels", "strip_kernels",
               "full_stage_maps")
BUILDERS = {"resnet50": lambda: models.deconv("resnet50", 17, False), "densenet121": lambda: models.fpn_densenet("densenet121", 17, False),
            "hg2": lambda: models.hg(17, 2)}


@functools.lru_cache(maxsize=None)
def _seeded(name, seed=5):
    torch.manual_seed(seed)
    return BUILDERS[name]()


@pytest.mark.parametrize("name, cls", [("densenet121", "FpnDensenet"), ("hg2", "HourglassNet")])
def test_non_resnet_models_are_hosts_without_the_resnet_trunk(name, cls):
    cls, m = getattr(models, cls), _seeded(name)
    assert type(m) is cls and issubclass(cls, PoseHost) and not issubclass(cls, models.PoseResnet)
    assert [a for a in RESNET_ONLY if hasattr(m, a)] == []
    assert not hasattr(m, "layer1") and m.supports_exact is False


def test_resnet_models_keep_their_switches_and_the_exact_mode_its_gate():
    for cls in (models.DeconvResnet, models.FpnResnet, models.LateralDeconvResnet):
        assert issubclass(cls, models.PoseResnet) and issubclass(models.PoseResnet, PoseHost)
        assert [a for a in RESNET_ONLY + ("fuse_stem_pool", "fuse_stem_pack") if not hasattr(cls, a)] == []
    assert issubclass(models.FpnResnet, models.FpnHead) and issubclass(models.FpnDensenet, models.FpnHead)
    assert hasattr(models.FpnDensenet, "fuse_stem_pool") and hasattr(models.FpnDensenet, "fuse_stem_pack")
    assert [c.supports_exact for c in (models.DeconvResnet, models.FpnResnet, models.LateralDeconvResnet, models.FpnDensenet, models.HourglassNet)] == \
        [True, False, False, False, False]


def test_models_is_the_drop_in_surface():
    names = ("deconv", "fpn", "fpn_densenet", "pose", "hg", "resnet_dict", "densenet_dict", "FPN_DENSENETS", "PoseHost", "PoseResnet", "DeconvResnet",
             "FpnHead", "FpnResnet", "FpnDensenet", "LateralDeconvResnet", "HourglassNet", "DenseLayer", "DenseBlock", "Transition", "HgBottleneck",
             "Hourglass", "_Stages", "_ExactHandle")
    assert [n for n in names if not hasattr(models, n)] == []
    assert all(callable(getattr(models, n)) for n in names[:5])
    assert set(models.resnet_dict) >= {50, 101, 152} and set(models.densenet_dict) == {121, 161, 169, 201}


def test_cached_is_a_memo_on_label_dtype_device():
    m = HipModule()
    made = []

    def make():
        made.append(object())
        return made[-1]
    cpu, meta = torch.device("cpu"), torch.device("meta")
    a = m._cached("conv1", torch.float16, cpu, make)
    assert m._cached("conv1", torch.float16, cpu, make) is a and m._cached("conv1", torch.float16, "cpu", make) is a and len(made) == 1
    others = [m._cached("conv2", torch.float16, cpu, make), m._cached("conv1", torch.float32, cpu, make), m._cached("conv1", torch.float16, meta, make)]
    assert len(made) == 4 and len({id(o) for o in others + [a]}) == 4
    assert set(m._layers) == {("conv1", torch.float16, "cpu"), ("conv2", torch.float16, "cpu"), ("conv1", torch.float32, "cpu"), ("conv1", torch.float16, "meta")}
    m._invalidate()
    assert m._layers == {}
    assert m._cached("conv1", torch.float16, cpu, make) is not a and len(made) == 5


@pytest.mark.parametrize("name", list(BUILDERS))
def test_construction_is_reproducible_under_a_seed(name):
    a = _seeded(name).state_dict()
    torch.manual_seed(5)
    b = BUILDERS[name]().state_dict()
    assert list(a) == list(b)
    assert [k for k in a if a[k].shape != b[k].shape or not torch.equal(a[k], b[k])] == []
    torch.manual_seed(6)
    c = BUILDERS[name]().state_dict()
    assert any(not torch.equal(a[k], c[k]) for k in a)          # (the seed is what the values follow)
