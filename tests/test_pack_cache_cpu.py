"""The contract of ``ops.cached_pack`` (no GPU): the memoised pack of a module's parameters is rebuilt, exactly once, after every
event that changes the parameter values -- the three forms of Adam.step() through the step hook ``configure_optimizers`` installs
(``ops.invalidate_packs``), in-place copies under ``no_grad`` and ``inference_mode``, ``load_state_dict``, the EMA swap in and
out -- and not rebuilt when nothing changed.

The fused Adam is the case that needs the hook: its step changes the values and leaves ``p._version`` where it was, so a key of
(data_ptr, _version) alone keeps serving the pack of the old weights."""
import pytest
import torch

from protein_redesign_amd import ops
from protein_redesign_amd.diffusion_model import _Ema


class Packed:
    """A small Linear, its pack (weight | bias as one tensor) through cached_pack, and the count of builds."""

    def __init__(self, seed=0):
        torch.manual_seed(seed)
        self.lin = torch.nn.Linear(5, 3)
        self.builds = 0

    def _build(self):
        self.builds += 1
        return torch.cat([self.lin.weight, self.lin.bias.unsqueeze(1)], dim=1).contiguous()

    def get(self):
        return ops.cached_pack(self.lin, "x", (self.lin.weight, self.lin.bias), self._build)

    def current(self):
        return torch.cat([self.lin.weight.detach(), self.lin.bias.detach().unsqueeze(1)], dim=1)

    def check_rebuilt_once(self, before, what):
        """After an event: ONE more build, the pack equals the current parameters, and a further call builds nothing."""
        n = self.builds
        got = self.get()
        assert self.builds == n + 1, f"{what}: {self.builds - n} builds after the change, expected exactly 1"
        assert torch.equal(got, self.current()), f"{what}: the pack does not hold the current parameters"
        assert not torch.equal(got, before), f"{what}: the parameters did not change -- the case checks nothing"
        assert self.get() is got and self.builds == n + 1, f"{what}: a second call without a change built again"
        return got


def test_two_calls_without_a_change_build_once():
    m = Packed()
    first = m.get()
    assert m.get() is first and m.get() is first and m.builds == 1
    assert torch.equal(first, m.current())


def _adam(params, **kw):
    opt = torch.optim.Adam(params, lr=1e-2, **kw)
    opt.register_step_post_hook(ops.invalidate_packs)            # what ProteinReDiffModel.configure_optimizers installs
    return opt


@pytest.mark.parametrize("form", ["fused", "foreach", "default"])
def test_rebuilt_after_every_adam_step(form):
    m = Packed(1)
    kw = {"fused": True} if form == "fused" else ({"foreach": True} if form == "foreach" else {})
    try:
        opt = _adam(m.lin.parameters(), **kw)
    except (RuntimeError, ValueError) as e:
        if form != "fused":
            raise
        pytest.skip(f"this torch cannot construct a fused Adam on CPU tensors: {e}")
    pack = m.get()
    x = torch.randn(4, 5)
    for step in range(3):                                        # every step, not only the first
        opt.zero_grad()
        m.lin(x).square().sum().backward()
        versions = [p._version for p in m.lin.parameters()]
        opt.step()
        print(f"Adam({form}) step {step}: _version {versions} -> {[p._version for p in m.lin.parameters()]}")
        pack = m.check_rebuilt_once(pack, f"Adam({form}).step() #{step}")


def test_configure_optimizers_installs_the_hook():
    """The optimiser the model hands out invalidates on step() by itself: no Fitter, no call by the user."""
    from protein_redesign_amd.constants import make_args
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    model = ProteinReDiffModel(make_args(single_dim=64, pair_dim=32, num_blocks=1, esm_dim=16, warmup_steps=2))
    opt = model.configure_optimizers()["optimizer"]
    lin = model.seq_mlp[1]
    builds = []
    get = lambda: ops.cached_pack(lin, "x", (lin.weight,), lambda: builds.append(1) or lin.weight.detach().clone())
    get()
    for p in model.parameters():
        p.grad = torch.ones_like(p) if p.requires_grad else None
    opt.step()
    assert torch.equal(get(), lin.weight.detach()) and len(builds) == 2
    get()
    assert len(builds) == 2


def test_fitter_invalidates_for_an_optimiser_without_the_hook():
    """training.Fitter tells the packs after the step of ANY optimiser it drives (here a fused Adam nobody hooked)."""
    from protein_redesign_amd import training
    from test_training_cpu import _StubModel
    model = _StubModel()
    try:
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, fused=True)
    except (RuntimeError, ValueError) as e:
        pytest.skip(f"this torch cannot construct a fused Adam on CPU tensors: {e}")
    lin = model.lin
    builds = []
    get = lambda: ops.cached_pack(lin, "x", (lin.weight,), lambda: builds.append(1) or lin.weight.detach().clone())
    get()
    training.Fitter(model, opt).step({"x": torch.randn(2, 6)}, 0)
    assert torch.equal(get(), lin.weight.detach()) and len(builds) == 2


@pytest.mark.parametrize("ctx", [torch.no_grad, torch.inference_mode])
def test_rebuilt_after_an_in_place_copy(ctx):
    m = Packed(2)
    pack = m.get()
    for k, p in enumerate(m.lin.parameters()):                   # each source on its own
        with ctx():
            p.copy_(torch.randn(p.shape))
        pack = m.check_rebuilt_once(pack, f"copy_ of source {k} under {ctx.__name__}")


def test_rebuilt_after_a_pack_built_under_inference_mode():
    """A pack built inside inference_mode (sample()) is dropped like any other when the parameters change afterwards."""
    m = Packed(3)
    with torch.inference_mode():
        pack = m.get()
    assert pack.is_inference() and m.get() is pack
    with torch.no_grad():
        m.lin.weight.mul_(1.5)
    m.check_rebuilt_once(pack, "mul_ after a build under inference_mode")


def test_rebuilt_after_load_state_dict():
    m, other = Packed(4), Packed(5)
    pack = m.get()
    m.lin.load_state_dict(other.lin.state_dict())
    got = m.check_rebuilt_once(pack, "load_state_dict")
    assert torch.equal(got, other.current())


def test_rebuilt_on_entering_and_leaving_the_ema_swap():
    m = Packed(6)
    params = list(m.lin.parameters())
    ema = _Ema(params, decay=0.5)
    with torch.no_grad():
        for p in params:
            p.add_(1.0)
    ema.update(params)                                           # the shadow now differs from the parameters
    pack = m.get()
    live = pack.clone()
    with ema.average_parameters(params):
        inside = m.check_rebuilt_once(pack, "EMA swap in")
        assert torch.equal(inside, torch.cat([ema.shadow[0], ema.shadow[1].unsqueeze(1)], dim=1))
    back = m.check_rebuilt_once(inside, "EMA swap out")
    assert torch.equal(back, live)


def test_invalidate_by_hand_covers_a_write_through_data():
    """The documented limit and its remedy: a write through ``p.data`` moves no version counter, so it is NOT seen;
    ``ops.invalidate_packs()`` is the public call for that."""
    m = Packed(7)
    pack = m.get()
    m.lin.weight.data.mul_(2.0)
    assert m.get() is pack and m.builds == 1                     # as documented: not seen
    ops.invalidate_packs()
    m.check_rebuilt_once(pack, "invalidate_packs() after a write through .data")
