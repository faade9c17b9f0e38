"""CPU (no GPU): FusedAdamW speaks torch's fused-optimizer GradScaler protocol (`_step_supports_amp_scaling`: the scaler
sets `grad_scale` / `found_inf` on the optimizer, calls step() and deletes them), the two C entry points behind it are
declared, exported, bound and refuse bad arguments before any HIP call, and the private torch hook `siglip_amd.GradScaler`
overrides still has the signature and the call site it was written against.  Nothing here launches a kernel."""
import ctypes as C
import inspect
import re

import pytest
import torch

OK, BAD_SHAPE, NULL = 0, -1, -5
D = 0x7F0000001000          # a 16-byte aligned dummy device pointer, never dereferenced


def _opt(pkg, **kw):
    return pkg.FusedAdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, **kw)


def test_protocol_attributes_and_step_signature(pkg):
    """Fails on the parent: no `_step_supports_amp_scaling`, and `grad_scale` is the 1/world float there."""
    opt = _opt(pkg)
    assert pkg.FusedAdamW._step_supports_amp_scaling is True and opt._step_supports_amp_scaling is True
    assert "grad_scaler" not in inspect.signature(opt.step).parameters      # that path is deprecated and warns
    assert list(inspect.signature(opt.step).parameters) == ["closure"]
    assert pkg.GradScaler is pkg.optim.GradScaler and issubclass(pkg.GradScaler, torch.amp.GradScaler)


def test_slots_cycle_as_gradscaler_step_uses_them(pkg):
    """The statements of GradScaler.step (torch/amp/grad_scaler.py), in its order, for both stages."""
    opt = _opt(pkg, grad_scale=0.25)             # the constructor keyword is the 1/world factor, stored privately
    assert opt._world_scale == 0.25
    scaler = torch.tensor(65536.0)
    for name in ("grad_scale", "found_inf"):
        assert not hasattr(opt, name)
        with pytest.raises(AttributeError):
            delattr(opt, name)
    # stage READY: the product with a scale the user set, 1 when there is none
    assert getattr(opt, "grad_scale", 1) == 1
    opt.grad_scale = scaler * getattr(opt, "grad_scale", 1)
    opt.found_inf = torch.tensor(0.0)
    assert torch.equal(opt.grad_scale, scaler) and opt.found_inf.item() == 0.0
    del opt.grad_scale
    del opt.found_inf
    assert getattr(opt, "grad_scale", 1) == 1 and getattr(opt, "found_inf", None) is None
    # stage UNSCALED: None stays None, and None is a set value that can be read and deleted
    opt.grad_scale = getattr(opt, "grad_scale", None)
    assert opt.grad_scale is None and hasattr(opt, "grad_scale")
    del opt.grad_scale
    assert not hasattr(opt, "grad_scale")
    for bad in (0.5, 1, "x"):
        with pytest.raises(TypeError):
            opt.grad_scale = bad
        with pytest.raises(TypeError):
            opt.found_inf = bad
    assert opt._world_scale == 0.25              # untouched by the slots


def test_constructor_keyword_is_unchanged(pkg):
    params = inspect.signature(pkg.FusedAdamW.__init__).parameters
    assert list(params) == ["self", "params", "lr", "betas", "eps", "weight_decay", "max_grad_norm", "grad_scale"]
    assert params["grad_scale"].default == 1.0 and params["max_grad_norm"].default is None
    assert _opt(pkg)._world_scale == 1.0
    # a state_dict round trip needs no device and keeps torch.optim.AdamW's layout
    opt = _opt(pkg)
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"}
    opt.load_state_dict(sd)


def test_torch_hook_signature_is_the_one_the_subclass_overrides(pkg):
    """`_check_inf_per_device` is private torch API: pin what siglip_amd.GradScaler relies on."""
    base = torch.amp.GradScaler
    assert list(inspect.signature(base._check_inf_per_device).parameters) == ["self", "optimizer"]
    assert list(inspect.signature(pkg.GradScaler._check_inf_per_device).parameters) == ["self", "optimizer"]
    src = inspect.getsource(base.step)
    assert "_step_supports_amp_scaling" in src
    assert re.search(r"stage\"\]\s+is\s+OptState\.READY:\s+self\._check_inf_per_device\(optimizer\)", src)
    assert 'getattr(optimizer, "grad_scale", 1)' in src and 'getattr(optimizer, "grad_scale", None)' in src
    assert "del optimizer.grad_scale" in src and "del optimizer.found_inf" in src
    body = inspect.getsource(base._check_inf_per_device)
    assert '["found_inf_per_device"]' in body and "_check_scale_growth_tracker" in body
    assert "found_inf_per_device" in inspect.getsource(base.update)
    # any other optimizer goes to the base class (a disabled scaler never reaches the hook)
    sc = pkg.GradScaler("cpu", enabled=False)
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.1)
    sgd.param_groups[0]["params"][0].grad = torch.ones(2)
    sc.step(sgd)
    assert torch.equal(sgd.param_groups[0]["params"][0].detach(), torch.full((2,), -0.1))


def test_symbols_are_declared_exported_and_bound(pkg, hiplib):
    declared = pkg.lib.declared_symbols()
    for name, nargs in (("sgl_op_grad_norm_amp", 11), ("sgl_op_adamw_amp", 14)):
        assert name in declared and hasattr(hiplib, name)
        assert len(getattr(hiplib, name).argtypes) == nargs
    assert hiplib.sgl_abi_version() == 3                               # new symbols only
    assert C.sizeof(pkg.lib.SglAmpState) == 32
    text = open(pkg.lib.HEADER_PATH).read()
    m = re.search(r"typedef struct \{([^}]*)\} sgl_amp_state;", text, flags=re.S)
    fields = re.findall(r"\b(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [n for n, _ in pkg.lib.SglAmpState._fields_]


def test_every_refusal_comes_before_a_launch(hiplib):
    def norm(table=D, bmap=D, nb=4, scale=D, inf=D, part=D, out=D, state=D):
        return hiplib.sgl_op_grad_norm_amp(table, bmap, nb, 1.0, 0.5, scale, inf, part, out, state, None)

    def adamw(table=D, aux=D, bmap=D, nb=4, step=1, hyper=None, ng=0, state=D):
        return hiplib.sgl_op_adamw_amp(table, aux, bmap, nb, 0.9, 0.999, 1e-8, step, D, hyper, ng, 0.0, state, None)

    for name in ("table", "bmap", "part", "out", "state"):
        assert norm(**{name: None}) == NULL
        assert norm(**{name: None}, nb=-1) == NULL                   # a NULL pointer is reported first
    for nb in (-1, 1 << 31):
        assert norm(nb=nb) == BAD_SHAPE
        assert norm(nb=nb, scale=None, inf=None) == BAD_SHAPE
    for name in ("scale", "inf", "state"):
        for off in (1, 2, 3):
            assert norm(**{name: D + off}) == BAD_SHAPE
    for name in ("table", "aux", "bmap", "state"):
        assert adamw(**{name: None}) == NULL
    for bad in (dict(nb=-1), dict(nb=1 << 31), dict(step=0), dict(step=-3), dict(ng=-1), dict(ng=17), dict(state=D + 2)):
        assert adamw(**bad) == BAD_SHAPE
    assert adamw(ng=2, hyper=None) == NULL
    assert adamw(nb=0) == OK                                         # empty plan: no launch
