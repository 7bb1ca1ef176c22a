"""The layer-level fixtures of the GPU suites: one seeded DAU layer, seeded device tensors, and the comparisons the suites share."""
import importlib

import pytest
import torch


def make_layer(S=8, F=16, cls=None, seed=0, mu=3.0, **kw):
    """DAUConv2d (or `cls`) of S -> F channels on the device, its parameters drawn after torch.manual_seed(seed): 2 x 2 units under
    kernel 9, offsets uniform in +-mu, a bias ~ N(0, 0.5^2) (bias_initializer=None: the layer's own zeros).  kw overrides any of it."""
    import dau_conv
    torch.manual_seed(seed)
    kw.setdefault("use_bias", True)
    kw.setdefault("mu_learning_rate_factor", 1.0)
    kw.setdefault("bias_initializer", dau_conv.random_normal_initializer(stddev=0.5))
    kw.setdefault("dau_units", (2, 2))
    kw.setdefault("max_kernel_size", 9)
    kw.setdefault("mu1_initializer", dau_conv.random_uniform_initializer(-mu, mu))
    if cls is not dau_conv.DAUConv1d:
        kw.setdefault("mu2_initializer", dau_conv.random_uniform_initializer(-mu, mu))
    return (cls or dau_conv.DAUConv2d)(filters=F, in_channels=S, **kw).cuda()


def rand(seed, shape, normal=False):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn if normal else torch.rand)(shape, device="cuda", generator=g)


def rand_x(seed, shape, dtype=torch.float32, memory_format=torch.contiguous_format):
    return rand(seed, shape).to(dtype).contiguous(memory_format=memory_format)


def rand_dy(seed, shape, dtype=torch.float32, memory_format=torch.contiguous_format):
    return rand(seed, shape, normal=True).to(dtype).contiguous(memory_format=memory_format)


def close(got, want, rel=2e-3):
    got, want = got.float(), want.float()
    assert torch.isfinite(got).all()
    err = ((got - want).abs() - rel * want.abs() - rel * want.abs().max()).max().item()
    assert err <= 0, "differs by %.3e (max |want| %.3e)" % ((got - want).abs().max().item(), want.abs().max().item())


def check_bias_grad(got, y, dy):
    """the bias gradient of a fused ReLU lies within 2^-16 * sum |dz| of the exact sum of dz = where(y <= 0, 0, dy)"""
    dz = torch.where(y <= 0, torch.zeros_like(dy), dy).double()
    exact, bound = dz.sum(dim=(0, 2, 3)), 2.0 ** -16 * dz.abs().sum(dim=(0, 2, 3))
    assert bool(((got.double() - exact).abs() <= bound).all()), ((got.double() - exact).abs().tolist(), bound.tolist())


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert bool(torch.isfinite(a.float()).all()), what
    assert torch.equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.numel())


@pytest.fixture(autouse=True)
def _leave_the_plan_cache_as_it_was():
    """the layer's plan cache is bounded and least-recently-used: the plans these tests add would push other modules' plans out of
    it (tests elsewhere compare its keys before and after a call), so each test takes its own out again.  (Autouse in the modules
    that import it, and in no other.)"""
    impl = importlib.import_module("dau_conv.dau_conv")
    before = set(impl._PLANS)
    yield
    for key in [k for k in impl._PLANS if k not in before]:
        impl._PLANS.pop(key).last_status()      # (a pending offset error would be raised here, not lost)
