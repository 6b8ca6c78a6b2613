"""``ProteinReDiffModel`` with the reference's LightningModule surface and a HIP hot path.

Mirrors reference ProteinReDiff/model.py:55-549 for everything ``generate.py`` / ``train.py`` touch:
constructor from Namespace|Mapping, ``add_argparse_args``, ``run_setup_schedule``, ``prepare_batch``
(eval branch), ``forward`` / ``sample_step`` (same signature, returns (noise_pred, seq_pred)),
``sample``, ``predict_step``, checkpoint hooks and ``state_dict`` key names.  The arithmetic of
``sample_step`` and of the reverse-diffusion loop runs in libprd_hip.so; nothing falls back to
PyTorch ops on the hot path.

Differences that are deliberate and documented:
* randomness is injected: every sample k draws its mask permutation and noise from a CPU fp32
  generator keyed (seed, global sample index) (``synthetic.NoiseSource``), so results do not depend
  on device RNG, batch size or on how samples are sharded over GPUs;
* the redesign mask is drawn per sample (identical to the reference at its default batch_size=1).
"""
from __future__ import annotations

import contextlib
import math
from argparse import ArgumentParser, Namespace
from typing import Dict, List, Mapping, Optional, Sequence, Union

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, ops
from .constants import ATOM_FEATURE_CARDS, BOND_FEATURE_CARDS, NUM_RESIDUE_CLASSES
from .schedule import reverse_coefficients, schedule_tables
from .conditioning import BATCH_KEY as SCAFFOLD_KEY, Scaffold, condition_rows_, level_table
from .guidance import MAX_N as GUIDE_MAX_N, Guidance, guide_eps_
from .masking import MaskDraws, Redesign
from .sequence import BATCH_KEY as RULES_KEY, SequenceRules, constrain_rows_
from .solver import Solver, check_time_dim, multistep_correct_, solver_boundary_
from .synthetic import NoiseSource
from .trunk import Denoiser, Linear

try:  # the reference subclasses pl.LightningModule (model.py:55); absent in this image
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # pragma: no cover - depends on the environment
    pl = None

    class _Base(nn.Module):
        """Minimal stand-in for pl.LightningModule: what model.py actually calls on ``self``."""

        def save_hyperparameters(self, args=None):
            self.hparams = args

        def log(self, *a, **k):
            pass

        @property
        def device(self):
            return next(self.parameters()).device

        @classmethod
        def load_from_checkpoint(cls, path, map_location="cpu", **overrides):
            ckpt = torch.load(path, map_location=map_location, weights_only=False)
            args = ckpt.get("hyper_parameters", {})
            args = dict(vars(args)) if isinstance(args, Namespace) else dict(args)
            if "args" in args and len(args) == 1:
                inner = args["args"]
                args = dict(vars(inner)) if isinstance(inner, Namespace) else dict(inner)
            args.update(overrides)
            model = cls(args)
            model.load_state_dict(ckpt["state_dict"])
            model.on_load_checkpoint(ckpt)
            return model


class _TableSum(nn.Module):
    """AtomEmbedding / BondEmbedding parameter container (modules.py:35-70): ``embeddings.{f}.weight``.
    The lookups are fused into prd_atom_embed / prd_static_pair."""

    def __init__(self, cards: Sequence[int], embed_dim: int):
        super().__init__()
        self.embeddings = nn.ModuleList([nn.Embedding(n, embed_dim) for n in cards])
        self.num_features = len(cards)
        self.scale = 1.0 / math.sqrt(self.num_features)


class AtomEmbedding(_TableSum):
    def __init__(self, embed_dim: int):
        super().__init__(ATOM_FEATURE_CARDS, embed_dim)


class BondEmbedding(_TableSum):
    def __init__(self, embed_dim: int):
        super().__init__(BOND_FEATURE_CARDS, embed_dim)


class RadialBasisProjection(nn.Module):
    """modules.py:73-82 (centres only; exp(-scale (d-c)^2) is generated inside prd_pair_init)."""

    def __init__(self, embed_dim: int, min_val: float = 0.0, max_val: float = 2.0):
        super().__init__()
        self.scale = (embed_dim - 1) / (max_val - min_val)
        self.center = nn.Parameter(torch.linspace(min_val, max_val, embed_dim), requires_grad=False)


class SinusoidalProjection(nn.Module):
    """modules.py:85-97 (frequencies only; sin/cos evaluated inside prd_time_embed)."""

    def __init__(self, embed_dim: int):
        super().__init__()
        if embed_dim % 2 != 0:
            raise ValueError(f"embed_dim must be even: {embed_dim}.")
        self.embed_dim = embed_dim
        self.weight = nn.Parameter(torch.logspace(-4.0, 0.0, embed_dim // 2), requires_grad=False)


class _Ema:
    """Shadow-parameter EMA with torch-ema 0.3's call surface and checkpoint format (model.py:124,194-201,217,238,250;
    environment.yml pins torch_ema==0.3): ``state_dict()`` carries decay / num_updates / shadow_params / collected_params,
    ``update()`` uses the warm-up decay min(decay, (1 + n) / (10 + n)).  The shadow list covers EVERY parameter in
    registration order (242 tensors for the reference configuration, as torch-ema 0.3 keeps them); checkpoints whose list
    only holds the 240 trainable tensors (the 0.2 behaviour) load as well."""

    def __init__(self, params, decay: float, use_num_updates: bool = True):
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.decay = decay
        self.num_updates = 0 if use_num_updates else None
        self.shadow = [p.detach().clone() for p in params]
        self.collected = None
        self.active = False          # becomes True once updated or loaded: until then shadow == init copy

    def to(self, device=None, dtype=None):
        self.shadow = [s.to(device=device) if device is not None else s for s in self.shadow]
        return self

    def _match(self, params):
        """Pairs (parameter, shadow) for a shadow list holding all parameters or only the trainable ones."""
        params = list(params)
        if len(self.shadow) == len(params):
            return list(zip(params, self.shadow))
        train = [p for p in params if p.requires_grad]
        if len(self.shadow) != len(train):
            raise ValueError(f"EMA holds {len(self.shadow)} shadow tensors, the model has {len(params)} parameters "
                             f"({len(train)} trainable)")
        return list(zip(train, self.shadow))

    def update(self, params):
        self.active = True
        decay = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            decay = min(decay, (1 + self.num_updates) / (10 + self.num_updates))
        with torch.no_grad():
            pairs = [(p.detach(), s) for p, s in self._match(params) if p.requires_grad]
            if pairs and all(p.device == s.device and p.is_cuda for p, s in pairs):
                # the same arithmetic as the loop below (s -= (s - p) * (1 - decay)) in three multi-tensor launches
                # instead of three launches per tensor (720 per optimisation step)
                shadow = [s for _, s in pairs]
                tmp = torch._foreach_sub(shadow, [p for p, _ in pairs])
                torch._foreach_mul_(tmp, 1.0 - decay)
                torch._foreach_sub_(shadow, tmp)
            else:
                for p, s in pairs:
                    s.sub_((s - p.to(s.device)) * (1.0 - decay))

    def state_dict(self):
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": self.shadow,
                "collected_params": self.collected}

    def load_state_dict(self, sd):
        shadow = sd.get("shadow_params")
        if shadow is not None:
            self.shadow = [s.detach().clone() for s in shadow]
            self.active = True
        self.decay = sd.get("decay", self.decay)
        self.num_updates = sd.get("num_updates", self.num_updates)
        self.collected = sd.get("collected_params")

    @contextlib.contextmanager
    def average_parameters(self, params=None):
        if not self.active or params is None:
            yield
            return
        pairs = self._match(params)
        saved = [p.detach().clone() for p, _ in pairs]
        with torch.no_grad():
            for p, s in pairs:
                p.copy_(s.to(p.device))
        try:
            yield
        finally:
            with torch.no_grad():
                for (p, _), s in zip(pairs, saved):
                    p.copy_(s)


class ProteinReDiffModel(_Base):
    def __init__(self, args: Union[Namespace, Mapping]):
        super().__init__()
        if isinstance(args, Mapping):
            args = Namespace(**args)
        self.pair_dim, self.single_dim = args.pair_dim, args.single_dim
        self.dist_dim, self.time_dim = args.dist_dim, args.time_dim
        self.max_bond_distance, self.max_relpos, self.esm_dim = args.max_bond_distance, args.max_relpos, args.esm_dim
        self.setup_schedule = False
        self.setup_esm = False
        self.mask_prob, self.num_steps = args.mask_prob, args.num_steps
        self.diffusion_schedule = args.diffusion_schedule
        self.learning_rate, self.warmup_steps, self.ema_decay = args.learning_rate, args.warmup_steps, args.ema_decay
        self.n_recycles, self.training_mode = args.n_recycles, args.training_mode
        # key of the injected randomness (see module docstring).  None = taken from torch's seeded global RNG
        # (torch.initial_seed(), i.e. what pl.seed_everything(args.seed) / generate.py --seed set) when a sample is drawn,
        # so different seeds give different samples like in the reference; set an int to pin it regardless of the global seed.
        self.sample_seed = None
        self.use_hip_graph = True               # replay one captured step graph inside sample()
        # What to do when a sampling loop / optimisation step ends with inf / NaN (the reference is fp32 end to end and cannot
        # overflow at 65504; the default split-16 arithmetic can -- include/prd_hip.h, OPERAND RANGE):
        #   "fp32"  (default) run the CALL again under PRD_ARITH_FP32 (a fresh call in this process, with a RuntimeWarning), and keep
        #           fp32 for this model's later calls; if that is non-finite too -- or the call already ran in fp32 -- raise;
        #   "raise" raise _lib.NonFiniteError naming the arithmetic;   "off" return whatever came out (no check, no host sync).
        self.nonfinite_policy = "fp32"
        self.arithmetic = None                  # None: the process default (_lib); "fp32" / "split16": this model's calls pin it
        self.arith_fallbacks = 0                # how many calls were repeated in fp32 by the policy above
        self.nonfinite_group = None             # process group over which a non-finite verdict is agreed (None: the default group)
        self._side = None                       # ops.SideStream of the device the model runs on (created on first use)
        self._sample_counter = 0
        self._mask_draw_counter = 0             # prepared batches that drew a training-mode mask (masking.MaskDraws)
        self.redesign: Optional[Redesign] = None    # design region of inference where no ``redesign=`` keyword is given (masking.Redesign)

        self.Denoiser = Denoiser(args)
        S, P = self.single_dim, self.pair_dim
        self.embed_atom_feats = AtomEmbedding(S)
        self.embed_beta = nn.Sequential(SinusoidalProjection(self.time_dim), Linear(self.time_dim, P, bias=False, init="normal"))
        self.embed_residue_type = nn.Sequential(
            nn.LayerNorm(NUM_RESIDUE_CLASSES, elementwise_affine=False),
            Linear(NUM_RESIDUE_CLASSES, S, bias=False, init="normal"), nn.ReLU())
        self.embed_bond_feats = BondEmbedding(P)
        self.embed_bond_distance = nn.Embedding(self.max_bond_distance + 1, P)
        self.embed_residue_esm = nn.Sequential(nn.LayerNorm(self.esm_dim, elementwise_affine=False),
                                               Linear(self.esm_dim, S, bias=False, init="normal"))
        self.embed_relpos = nn.Embedding(self.max_relpos * 2 + 1, P)
        self.embed_dist = nn.Sequential(RadialBasisProjection(self.dist_dim), Linear(self.dist_dim, P, bias=False, init="normal"))
        self.weight_radial = nn.Sequential(nn.LayerNorm(P, elementwise_affine=False), Linear(P, P, init="relu"),
                                           nn.ReLU(), Linear(P, 1, bias=False, init="final"))
        self.seq_mlp = nn.Sequential(nn.LayerNorm(S, elementwise_affine=False), Linear(S, S, init="relu"), nn.ReLU(),
                                     Linear(S, NUM_RESIDUE_CLASSES, bias=False, init="final"))
        self.ema = _Ema(self.parameters(), decay=self.ema_decay)
        self.save_hyperparameters(args)

    # ------------------------------------------------------------------ argparse (model.py:130-170)
    @staticmethod
    def add_argparse_args(parent_parser: ArgumentParser) -> ArgumentParser:
        g = parent_parser.add_argument_group("DiffusionModel")
        g.add_argument("--training_mode", action="store_true")
        for name, typ, default in (
                ("mask_prob", float, 1.0), ("esm_dim", int, 1280), ("time_dim", int, 256), ("dist_dim", int, 256),
                ("single_dim", int, 512), ("pair_dim", int, 64), ("head_dim", int, 16), ("num_heads", int, 4),
                ("transition_factor", int, 4), ("num_blocks", int, 12), ("max_bond_distance", int, 7),
                ("max_relpos", int, 32), ("num_steps", int, 64), ("diffusion_schedule", str, "linear"),
                ("learning_rate", float, 4e-4), ("warmup_steps", int, 1000), ("ema_decay", float, 0.999)):
            g.add_argument(f"--{name}", type=typ, default=default)
        g2 = parent_parser.add_argument_group("IterativeDenoiser")   # parsed, unused
        for name, typ, default in (
                ("n_recycles", int, 4), ("top_k_neighbors", int, 30), ("dropout", float, 0.3),
                ("num_gvp_encoder_layers", int, 3), ("num_positional_embeddings", int, 16),
                ("gvp_edge_hidden_dim_scalar", int, 32), ("gvp_edge_hidden_dim_vector", int, 32)):
            g2.add_argument(f"--{name}", type=typ, default=default)
        return parent_parser

    # ------------------------------------------------------------------ schedule / hooks
    def run_setup_schedule(self):
        dev = self.device
        for k, v in schedule_tables(self.num_steps, self.diffusion_schedule).items():
            setattr(self, k, v.to(dev))
        self._coef = reverse_coefficients({k: getattr(self, k).cpu() for k in
                                           ("alphas", "sqrt_one_minus_alphas_cumprod", "sqrt_alphas", "sqrt_betas")}).to(dev)

    def to(self, *args, **kwargs):
        out = torch._C._nn._parse_to(*args, **kwargs)
        self.ema.to(device=out[0], dtype=out[1])
        self.setup_schedule = False
        return super().to(*args, **kwargs)

    def on_save_checkpoint(self, checkpoint):
        checkpoint["ema_state_dict"] = self.ema.state_dict()

    def on_load_checkpoint(self, checkpoint):
        if "ema_state_dict" in checkpoint:
            self.ema.load_state_dict(checkpoint["ema_state_dict"])

    def configure_optimizers(self):
        # the reference's Adam (model.py:203-217); on the GPU its fused single-kernel form (same update rule, one launch instead of a
        # dozen multi-tensor passes over the 16 M parameters: 0.6 -> 0.2 ms per step)
        params = list(self.parameters())
        fused = bool(params) and all(p.is_cuda and p.is_floating_point() for p in params)
        optimizer = torch.optim.Adam(params, lr=self.learning_rate, **({"fused": True} if fused else {}))
        # the fused step writes the parameters without moving their version counter: the packed weights (ops.cached_pack) are
        # told here, whoever calls step()
        optimizer.register_step_post_hook(ops.invalidate_packs)
        sched = torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=1.0 / self.warmup_steps,
                                                  total_iters=self.warmup_steps - 1)
        return {"optimizer": optimizer, "lr_scheduler": {"scheduler": sched, "interval": "step"}}

    def optimizer_step(self, *args, **kwargs):
        if pl is not None:
            super().optimizer_step(*args, **kwargs)
        self.ema.update(self.parameters())

    # ------------------------------------------------------------------ loss path (model.py:471-549), forward only
    def q(self, x, seq, t, noise_z, noise_seq, batch):
        """Forward noising of structure / sequence at step t and of the sequence at t-1 (model.py:471-488)."""
        ac, om = self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod
        extra, inv = batch["residue_extra_mask"], batch["residue_inv_extra_mask"]
        z_t = ac[t][:, None, None] * x + om[t][:, None, None] * noise_z
        seq_t = ac[t][:, None, None] * seq + om[t][:, None, None] * noise_seq
        seq_t = extra.unsqueeze(-1) * seq + inv.unsqueeze(-1) * seq_t
        t1 = (t - 1).clamp(min=0)
        seq_t1 = ac[t1][:, None, None] * seq + om[t1][:, None, None] * noise_seq
        return z_t, seq_t, seq_t1, t1

    def diffusion_loss(self, batch, x, mask, t, noise_z=None, noise_seq=None):
        """model.py:490-526.  The network forward runs on the HIP path; the O(N) loss reductions are torch ops.
        ``noise_z`` / ``noise_seq`` (mean-free) may be injected; otherwise they are drawn on the device."""
        seq, rm = batch["residue_one_hot"], batch["residue_mask"]
        if noise_z is None:
            noise_z = ops.remove_mean(torch.randn_like(x), mask.contiguous())
        if noise_seq is None:
            noise_seq = ops.remove_mean(torch.randn_like(seq), rm.contiguous())
        z_t, seq_t, seq_t1, t1 = self.q(x, seq, t, noise_z, noise_seq, batch)
        noise_pred, seq_pred = self(batch, z_t, seq_t, mask, t)
        ac, om = self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod
        seq_pred_t1 = ac[t1][:, None, None] * seq_pred + om[t1][:, None, None] * noise_seq
        loss = (mask.unsqueeze(-1) * torch.square(noise_pred - noise_z)).sum(dim=(1, 2))
        loss = loss + F.kl_div(torch.log_softmax(seq_pred_t1, dim=-1) * rm.unsqueeze(-1),
                               torch.softmax(seq_t1, dim=-1) * rm.unsqueeze(-1), reduction="none").sum()
        ce = F.cross_entropy(((seq_pred + 1) / 2).view(-1, NUM_RESIDUE_CLASSES), batch["residue_type"].view(-1),
                             reduction="none", ignore_index=0)
        return loss + (ce * mask.view(-1)).sum()

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """model.py:226-247: loss under the EMA weights, logged as ``val_loss``."""
        if not self.setup_schedule:
            self.run_setup_schedule()
            self.setup_schedule = True
        batch = self.prepare_batch(batch, batch_idx)
        x, mask = batch["x"], batch["residue_and_atom_mask"]
        num_nodes = (mask > 0.5).sum(-1)
        t = torch.randint(0, self.num_steps, size=(x.size(0),), device=x.device)
        with self.ema.average_parameters(self.parameters()):
            diff_loss = self.diffusion_loss(batch, x, mask, t)
        loss = torch.mean(diff_loss / num_nodes)
        self.log("val_loss", loss, on_epoch=True, sync_dist=True, batch_size=x.size(0))
        return loss

    def training_step(self, batch, batch_idx, t=None, noise_z=None, noise_seq=None, sources=None, check_finite=True, mask_draws=None):
        """model.py:528-549: mean over the batch of diffusion_loss / node count, differentiable with respect to every trainable
        parameter (training.network: HIP forward, per-operator backward, per-block recompute).  ``t`` / the noises / the mask
        sources may be injected (parity tests); otherwise they are drawn like the reference draws them.  ``sources`` feed the
        eval-branch mask, ``mask_draws`` (masking.MaskDraws) the training-mode one (``training_mode=True``)."""
        self.check_widths()
        if not self.setup_schedule:
            self.run_setup_schedule()
            self.setup_schedule = True
        if sources is None and not self.training_mode:
            # the reference draws a fresh torch.randperm at every optimisation step (model.py:460 -> mask_utils.py:87), so the
            # redesign mask of a complex differs from epoch to epoch: key the draw on a running count of training steps
            # (batch_idx restarts every epoch; keyed determinism on batch_idx is for validation / predict only)
            sources = self._sources(batch["atom_mask"].shape[0], None)
        batch = self.prepare_batch(batch, batch_idx, sources=sources, mask_draws=mask_draws)
        x, mask = batch["x"], batch["residue_and_atom_mask"]
        num_nodes = (mask > 0.5).sum(-1)
        if t is None:
            t = torch.randint(0, self.num_steps, size=(x.size(0),)).to(x.device)
        if noise_z is None:                     # drawn HERE so that a repeated forward (non-finite policy) sees the same noise
            noise_z = ops.remove_mean(torch.randn_like(x), mask.contiguous())
        if noise_seq is None:
            noise_seq = ops.remove_mean(torch.randn_like(batch["residue_one_hot"]), batch["residue_mask"].contiguous())

        def forward_loss():
            return torch.mean(self.diffusion_loss(batch, x, mask, t, noise_z, noise_seq) / num_nodes)

        with _lib.arithmetic(self.arithmetic):
            loss = forward_loss()
        if check_finite and self.nonfinite_policy != "off" and loss.is_cuda and self._any_rank(not bool(torch.isfinite(loss.detach()))):
            loss = self._nonfinite_training_step(forward_loss)
        self.log("train_loss", loss, on_step=True, on_epoch=True, sync_dist=True, batch_size=x.size(0))
        return loss

    def _current_arith(self) -> int:
        return _lib.GEMM_MODES[self.arithmetic] if self.arithmetic is not None else _lib.arith()

    def _any_rank(self, flag: bool) -> bool:
        """``flag`` OR-ed over the data-parallel ranks (``self.nonfinite_group``, default: the default process group) so that every
        rank takes the SAME branch of the non-finite policy: a rank that alone switched arithmetic would train a different model, and
        a rank that alone raised would leave the others waiting in the gradient all-reduce."""
        if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            return flag
        group = getattr(self, "nonfinite_group", None)
        if torch.distributed.get_world_size(group) < 2:
            return flag
        dev = self.device if torch.distributed.get_backend(group) == "nccl" else "cpu"
        f = torch.tensor([1.0 if flag else 0.0], device=dev)
        torch.distributed.all_reduce(f, op=torch.distributed.ReduceOp.MAX, group=group)
        return bool(f.item() != 0)

    def _nonfinite_training_step(self, forward_loss):
        """The loss of a training step came out inf / NaN (on this rank or on another one: ``_any_rank``).  Under split-16 arithmetic
        with policy "fp32": THIS MODEL is pinned to PRD_ARITH_FP32 from here on (``self.arithmetic``, as sample()'s fallback does; the
        process default is left alone) and the forward is repeated under it.  The backward of the returned loss runs after this
        function returns; every autograd node of training.py records the arithmetic of its forward and re-enters it in its backward
        (training._pin_arithmetic), so the fp32 forward gets fp32 recomputes and fp32 backward kernels.  Anything else raises."""
        import warnings
        cur = self._current_arith()
        if cur == 1 and self.nonfinite_policy == "fp32":
            warnings.warn("training_step: non-finite loss under split-16 arithmetic (an operand beyond the fp16 range: include/prd_hip.h, "
                          "OPERAND RANGE); pinning this model to PRD_ARITH_FP32 and repeating the step", RuntimeWarning, stacklevel=3)
            self.arithmetic = "fp32"
            self.arith_fallbacks += 1
            with _lib.arithmetic("fp32"):
                loss = forward_loss()
            if not self._any_rank(not bool(torch.isfinite(loss.detach()))):
                return loss
            cur = 0
        raise _lib.NonFiniteError(f"training_step: non-finite loss under {_lib.ARITH_NAMES[cur]} arithmetic"
                                  + (" (the fp32 repeat of a non-finite split-16 step)" if self.arith_fallbacks and cur == 0 else "")
                                  + (": outside the operand range of the split arithmetic (include/prd_hip.h); set model.arithmetic = 'fp32' "
                                     "or nonfinite_policy = 'fp32'" if cur == 1 else ": the weights / inputs themselves produce inf or NaN"))

    def predict_step(self, batch, batch_idx, redesign: Optional[Redesign] = None, scaffold: Optional[Scaffold] = None,
                     sequence_rules: Optional[SequenceRules] = None, solver: Optional[Solver] = None,
                     guidance: Optional[Guidance] = None):
        kw = {} if scaffold is None else {"scaffold": scaffold}
        if sequence_rules is not None:
            kw["sequence_rules"] = sequence_rules
        if solver is not None:
            kw["solver"] = solver
        if guidance is not None:
            kw["guidance"] = guidance
        with self.ema.average_parameters(self.parameters()):
            return self.sample(batch, batch_idx=batch_idx, redesign=redesign, **kw)

    # ------------------------------------------------------------------ batch preparation (model.py:424-468)
    def _sources(self, b: int, batch_idx: Optional[int] = None) -> List[NoiseSource]:
        """Default noise sources of a batch of b samples: keyed (seed, global sample index).  The seed follows the seeded
        global RNG unless ``sample_seed`` pins it; the index interleaves the ranks of an initialised process group
        (dataloader batch ``batch_idx`` of rank r holds samples (batch_idx * world + r) * b ...), so that ranks of a
        multi-GPU ``Trainer.predict`` never draw the same sample twice (the reference's identically seeded ranks do)."""
        seed = self.sample_seed if self.sample_seed is not None else (torch.initial_seed() & 0x7FFFFFFF)
        world, rank = 1, 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            world, rank = torch.distributed.get_world_size(), torch.distributed.get_rank()
        if batch_idx is None:           # direct sample() calls: running count of the samples this object has drawn
            first = self._sample_counter * world + rank * b
            self._sample_counter += b
        else:
            first = (int(batch_idx) * world + rank) * b
        return [NoiseSource(seed, first + k) for k in range(b)]

    def _mask_draws(self) -> MaskDraws:
        """Default draws of a training-mode mask: keyed (seed, running count of the batches this object has prepared), the ranks
        of an initialised process group interleaved -- a fresh mask at every optimisation step, as the reference draws it."""
        seed = self.sample_seed if self.sample_seed is not None else (torch.initial_seed() & 0x7FFFFFFF)
        world, rank = 1, 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            world, rank = torch.distributed.get_world_size(), torch.distributed.get_rank()
        index = self._mask_draw_counter * world + rank
        self._mask_draw_counter += 1
        return MaskDraws(seed, index)

    def _training_mode_mask(self, batch, mask_draws: Optional[MaskDraws]):
        """model.py:442-455: one of three masks per prepared batch -- random (rt < 0.3, p = scale * u), spatial (0.3 <= rt < 0.5,
        p = linspace(0, u, 1000)[idx]) or none -- with u = uniform(0.1, mask_prob).  The draws come from the host
        (masking.MaskDraws: nothing drawn depends on device data), the selection is ONE launch of prd_mask_lowest_k on the current
        stream: no device-to-host synchronisation, unlike the eval branch below.  ``residue_esm_tokens`` is optional (the reference
        masks it and never reads the result): masked in place when present, in the two branches where the reference does."""
        rm = batch["residue_mask"].contiguous()
        b, N = rm.shape
        dev = rm.device
        d = (mask_draws if mask_draws is not None else self._mask_draws()).draw(b, N, self.mask_prob)

        def upload(t):      # an ordinary asynchronous copy: pinned staging, ordered on the current stream
            return t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t.to(dev)

        p = upload(torch.full((b,), d.fraction, dtype=torch.float64).to(torch.float32))
        tokens = batch.get("residue_esm_tokens") if d.branch != "none" else None     # model.py:455 leaves the tokens alone
        if tokens is not None and not (tokens.dtype == torch.int64 and tokens.is_contiguous()):
            raise ValueError("residue_esm_tokens must be a contiguous int64 tensor [b, N] (it is masked in place)")
        if d.branch == "spatial":
            return ops.mask_lowest_k(rm, p, atom_pos=batch["atom_pos"].contiguous(), atom_mask=batch["atom_mask"].contiguous(),
                                     ca_pos=batch["residue_atom_pos"][:, :, 1], tokens=tokens)
        # "random", and "none" as its p = 0 case (k = 0: extra = residue_mask, inv = 0; the keys are not read)
        return ops.mask_lowest_k(rm, p, key=upload(d.keys) if d.keys is not None else rm, tokens=tokens)

    def _prepare_batch_training_mode(self, batch, mask_draws: Optional[MaskDraws]):
        """model.py:426-458, 464-468 with the mask of ``_training_mode_mask``: the same assignments as the eval branch."""
        am, rm = batch["atom_mask"], batch["residue_mask"]
        one_hot = F.one_hot(batch["residue_type"], num_classes=NUM_RESIDUE_CLASSES) * 2.0 - 1.0
        pos = am.unsqueeze(-1) * batch["atom_pos"] + rm.unsqueeze(-1) * batch["residue_atom_pos"][:, :, 1]
        extra, inv = self._training_mode_mask(batch, mask_draws)
        batch["residue_one_hot"] = one_hot * extra.unsqueeze(-1)
        batch["residue_esm"] = batch["residue_esm"] * extra.unsqueeze(-1)
        batch["residue_type_masked"] = (batch["residue_type"] * extra).long()
        batch["residue_extra_mask"] = extra
        batch["residue_inv_extra_mask"] = inv
        batch["x"] = 0.1 * pos
        batch["residue_and_atom_mask"] = am + rm
        return batch

    def _redesign_spec(self, redesign: Optional[Redesign]) -> Optional[Redesign]:
        """The design region in force: the keyword, else ``self.redesign``, else None (the reference's random subset).  The
        training recipe draws its own masks: a spec under ``training_mode=True`` is an error."""
        spec = redesign if redesign is not None else self.redesign
        if spec is None:
            return None
        if not isinstance(spec, Redesign):
            raise TypeError(f"redesign must be a masking.Redesign, got {type(spec).__name__}")
        if self.training_mode:
            raise ValueError("a redesign region applies to inference; under training_mode=True the training recipe draws its own masks")
        return spec

    def _scaffold_spec(self, scaffold: Optional[Scaffold]) -> Optional[Scaffold]:
        """The scaffold of a call: the keyword or None -- there is no attribute.  Conditioning holds rows to the input structure at
        inference; the training recipe noises every row: a scaffold under ``training_mode=True`` is an error."""
        if scaffold is None:
            return None
        if not isinstance(scaffold, Scaffold):
            raise TypeError(f"scaffold must be a conditioning.Scaffold, got {type(scaffold).__name__}")
        if self.training_mode:
            raise ValueError("a scaffold conditions inference on the input structure; under training_mode=True it is refused")
        if scaffold.start is not None and scaffold.start >= self.num_steps:
            raise ValueError(f"Scaffold: start must be a level in [0, {self.num_steps - 1}] (num_steps = {self.num_steps}), got {scaffold.start}")
        return scaffold

    def _rules_spec(self, rules: Optional[SequenceRules]) -> Optional[SequenceRules]:
        """The sequence rules of a call: the keyword or None -- there is no attribute.  Rules say what inference may design; the
        training recipe learns from the data's own sequence: rules under ``training_mode=True`` are an error."""
        if rules is None:
            return None
        if not isinstance(rules, SequenceRules):
            raise TypeError(f"sequence_rules must be a sequence.SequenceRules, got {type(rules).__name__}")
        if self.training_mode:
            raise ValueError("sequence rules constrain what inference designs; under training_mode=True they are refused")
        return rules

    def _solver_spec(self, solver: Optional[Solver], scaffold: Optional[Scaffold] = None) -> Optional[Solver]:
        """The solver of a call: the keyword or None -- there is no attribute.  A solver chooses the levels inference visits; the
        training recipe draws its own: a solver under ``training_mode=True`` is an error.  Everything host data decides is decided
        here, before any library call: the time embedding the boundary kernel holds, and that the levels fit this model's schedule
        and the scaffold's starting level."""
        if solver is None:
            return None
        if not isinstance(solver, Solver):
            raise TypeError(f"solver must be a solver.Solver, got {type(solver).__name__}")
        if self.training_mode:
            raise ValueError("a solver chooses the levels inference visits; under training_mode=True it is refused")
        check_time_dim(self.time_dim)
        solver.levels(self.num_steps, scaffold.start if scaffold is not None else None, self.diffusion_schedule)
        return solver

    def _guidance_spec(self, guidance: Optional[Guidance], solver: Optional[Solver] = None) -> Optional[Guidance]:
        """The guidance of a call: the keyword or None -- there is no attribute.  Guidance steers inference; the training recipe noises
        and denoises the data as it is: guidance under ``training_mode=True`` is an error.  prd_guide_eps sits between the network and a
        boundary that takes the raw output of the coordinate head, which only the fused boundaries do: the un-fused form
        (PRD_FUSED_BOUNDARY=0, or a time_dim above 512 without a solver) is refused.  Host data only: no library call."""
        if guidance is None:
            return None
        if not isinstance(guidance, Guidance):
            raise TypeError(f"guidance must be a guidance.Guidance, got {type(guidance).__name__}")
        if self.training_mode:
            raise ValueError("guidance steers the coordinates of inference; under training_mode=True it is refused")
        import os
        if solver is None and (os.environ.get("PRD_FUSED_BOUNDARY", "1") == "0" or not ops.step_boundary_fusable(self.time_dim)):
            raise ValueError("guidance needs the fused step boundary, which takes the coordinate head's raw output: it is refused under "
                             f"PRD_FUSED_BOUNDARY=0 and, without a solver, for a time_dim above 512 (this model has time_dim = "
                             f"{self.time_dim}, PRD_FUSED_BOUNDARY={os.environ.get('PRD_FUSED_BOUNDARY', '1')})")
        guidance.check_rows(GUIDE_MAX_N, "the library's rows")      # the batch's own N is checked when the loop knows it
        return guidance

    def _redesign_mask(self, batch, spec: Redesign):
        """(extra, inv) of a design region, built on the device without a host synchronisation.  ``within`` / ``nearest``: ONE
        launch of prd_mask_lowest_k (PRD_MASK_LIGAND_WITHIN / _NEAREST) keyed on the distance of every C-alpha to the nearest
        ligand atom; ``positions``: two elementwise products with ``residue_mask``."""
        rm = batch["residue_mask"].contiguous()
        b, N = rm.shape
        if spec.kind == "positions":
            m = spec.mask
            if m.shape[-1] != N or (m.dim() == 2 and m.shape[0] not in (1, b)):
                raise ValueError(f"Redesign.positions: a mask of shape {tuple(m.shape)} does not fit a batch of shape {(b, N)}")
            spec = spec.to(rm.device)
            return rm * spec.keep, rm * spec.mask
        p = torch.full((b,), spec.value, dtype=torch.float32, device=rm.device)
        return ops.mask_lowest_k(rm, p, atom_pos=batch["atom_pos"].contiguous(), atom_mask=batch["atom_mask"].contiguous(),
                                 ca_pos=batch["residue_atom_pos"][:, :, 1], ligand=spec.kind)

    def prepare_batch(self, batch, id=None, sources: Optional[Sequence] = None, mask_draws: Optional[MaskDraws] = None,
                      redesign: Optional[Redesign] = None):
        """Eval branch (:459-468): ``int(n_res * mask_prob)`` residues per sample leave the known set, chosen on the host from
        ``sources`` -- or, with a design region (``redesign=`` / ``self.redesign``, masking.Redesign: the pocket within a radius of
        the ligand, the fraction of residues nearest to it, or explicit positions), the residues of that region, selected on the
        device (``_redesign_mask``; ``sources`` and ``mask_prob`` are then not used for the mask).  Training-mode branch (:442-458, ``training_mode=True``, the paper's recipe ``--training_mode``): a
        stochastic random mask, a spatial mask around the ligand centroid, or none, drawn per prepared batch from ``mask_draws``
        (default: keyed on a running count) and selected on the device (``_training_mode_mask``).  Deviations from the reference
        (DESIGN.md §7): the random branch takes int(count * p) residues PER SAMPLE (the reference flattens the batch; equal at
        batch size 1), and k never exceeds a sample's own residue count.  ``residue_esm_tokens`` is optional."""
        spec = self._redesign_spec(redesign)
        if self.training_mode:
            return self._prepare_batch_training_mode(batch, mask_draws)
        am, rm = batch["atom_mask"], batch["residue_mask"]
        dev = am.device
        b = am.shape[0]
        if spec is None and sources is None:
            sources = self._sources(b, id if isinstance(id, int) else None)
        one_hot = F.one_hot(batch["residue_type"], num_classes=NUM_RESIDUE_CLASSES) * 2.0 - 1.0
        pos = am.unsqueeze(-1) * batch["atom_pos"] + rm.unsqueeze(-1) * batch["residue_atom_pos"][:, :, 1]
        if spec is not None:
            extra, inv = self._redesign_mask(batch, spec)
        else:
            rm_cpu = rm.detach().cpu()
            extra = rm_cpu.clone()
            inv = torch.zeros_like(rm_cpu)
            for k in range(b):        # RandomMaskingModule(stochastic=False), per sample (mask_utils.py:77-102)
                ones = torch.where(rm_cpu[k] == 1)[0]
                n = int(ones.numel() * self.mask_prob)
                sel = ones[sources[k].randperm(ones.numel())[:n]]
                extra[k, sel] = 0
                inv[k, sel] = 1
            extra, inv = extra.to(dev), inv.to(dev)
        batch["residue_one_hot"] = one_hot * extra.unsqueeze(-1)
        batch["residue_esm"] = batch["residue_esm"] * extra.unsqueeze(-1)
        batch["residue_type_masked"] = (batch["residue_type"] * extra).long()
        batch["residue_extra_mask"] = extra
        batch["residue_inv_extra_mask"] = inv
        batch["x"] = 0.1 * pos
        batch["residue_and_atom_mask"] = am + rm
        return batch

    # ------------------------------------------------------------------ the network (model.py:254-375)
    def _static_inputs(self, batch) -> Dict[str, torch.Tensor]:
        """Step-invariant embeddings: computed once per ``sample``."""
        am, rm = batch["atom_mask"].contiguous(), batch["residue_mask"].contiguous()
        S, P = self.single_dim, self.pair_dim
        bond_tabs = [e.weight for e in self.embed_bond_feats.embeddings]
        sp = ops.static_pair({k: batch[k].contiguous() for k in (
            "atom_mask", "residue_mask", "bond_mask", "bond_feats", "bond_distance", "residue_index",
            "residue_chain_index")}, bond_tabs + [self.embed_bond_distance.weight, self.embed_relpos.weight],
            self.max_bond_distance, self.max_relpos, P)
        tabs = torch.cat([e.weight for e in self.embed_atom_feats.embeddings], dim=0).contiguous()
        offsets = getattr(self, "_atom_table_offsets", None)
        if offsets is None or offsets.device != am.device:             # constant: uploaded once (not a host copy per call)
            offs, acc = [], 0
            for n in ATOM_FEATURE_CARDS:
                offs.append(acc)
                acc += n
            offsets = self._atom_table_offsets = torch.tensor(offs, dtype=torch.int32, device=am.device)
        ss = ops.atom_embed(batch["atom_feats"].contiguous(), am, tabs, offsets, S)
        esm = ops.layer_norm(batch["residue_esm"].contiguous())
        ss = ops.linear(esm, self.embed_residue_esm[1].weight, rowmask=rm, resid=ss)
        return {"pair": sp, "single": ss}

    def _step_inputs(self, static, seq_t, rm, t):
        """Per-step inputs of the network that do not depend on the coordinates: single (model.py:343-346) and the time
        embedding (model.py:341, 360).  Inside ``sample()`` the fused step-boundary kernel produces them for the next step."""
        single = ops.single_init(static["single"], seq_t.contiguous(), rm, self.embed_residue_type[1].weight)
        eb = ops.time_embed(t.contiguous(), self.embed_beta[0].weight, self.embed_beta[1].weight, self.num_steps)
        return single, eb

    def _network(self, batch, z, seq_t, mask, t, static=None, step_inputs=None, raw_noise=False, defer_seq_head=False):
        """``step_inputs`` = (single, ebeta) if already computed; ``raw_noise``: return the coordinate head's output before
        remove_mean (the step-boundary kernel removes the mean itself); ``defer_seq_head``: return the sequence head's HIDDEN units
        instead of the logits (the step-boundary kernel applies the last layer itself)."""
        den = self.Denoiser
        self.check_widths()                     # before the first launch, with the supported set
        if z.is_cuda and not ops.default_head_layout(den.num_heads, den.head_dim):
            ops.check_head_layout(den.num_heads, den.head_dim, den.pair_dim)     # before the first launch, with the supported set
        if static is None:
            static = self._static_inputs(batch)
        rm = batch["residue_mask"].contiguous()
        mask = mask.contiguous()
        z = z.contiguous()
        side = self._side
        if side is None or side.stream is not None and side.stream.device != z.device:
            side = self._side = ops.SideStream(z.device)
        if step_inputs is None:
            step_inputs = self._step_inputs(static, seq_t, rm, t)
        single, eb = step_inputs
        # (opt-in, measured slower: ops.SideStream) the single-only chain beside the pair input stage, joined at the OPM
        with side.fork():
            pre = self.Denoiser.project_single(single, mask)
        sm = self.seq_mlp
        # the pair input stage runs inside Denoiser.run_ (fused with the outer-product update and the first bias heads); the
        # sequence head's first layer is linear in LN(single_out), like the last block's outer-linear term: one launch for both
        single, pair, h = self.Denoiser.run_(single, None, mask, pre=pre, join=side.join, tail=(sm[1].weight, sm[1].bias),
                                             pair_init=(static["pair"], z, self.embed_dist[0].center, self.embed_dist[1].weight, eb))
        with side.fork():
            if h is None:
                h = ops.linear(single, sm[1].weight, sm[1].bias, act=1, ln_a=True)    # LayerNorm (no affine) fused into the linear
            seq_pred = h if defer_seq_head else ops.linear(h, sm[3].weight)
        wr = self.weight_radial
        eps_raw = ops.coord_head(pair, z, mask, wr[1].weight, wr[1].bias, wr[3].weight)
        noise_pred = eps_raw if raw_noise else ops.remove_mean(eps_raw, mask)
        side.join()
        return noise_pred, seq_pred

    def check_widths(self) -> None:
        """ValueError naming the supported set when a width of this model does not run on the GPU (ops.check_model_widths;
        host-only: no library call)."""
        ops.check_model_widths(dict(single_dim=self.single_dim, pair_dim=self.pair_dim, dist_dim=self.dist_dim, time_dim=self.time_dim,
                                    esm_dim=self.esm_dim, transition_factor=self.Denoiser.transition_factor))

    def forward(self, batch, z, seq_t, mask, t):
        """Inference (no_grad / inference_mode): the fused HIP path.  With autograd enabled: the same HIP operators, one
        autograd node each (training.py), so that ``diffusion_loss(...).backward()`` reaches every parameter."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from . import training
            return training.network(self, batch, z, seq_t, mask, t)
        return self._network(batch, z, seq_t, mask, t)

    def sample_step(self, batch, z, seq_t, mask, t):
        return self._network(batch, z, seq_t, mask, t)

    # ------------------------------------------------------------------ reverse diffusion (model.py:377-422)
    @torch.inference_mode()
    def sample(self, batch, sources: Optional[Sequence] = None, batch_idx: Optional[int] = None, mask_draws: Optional[MaskDraws] = None,
               redesign: Optional[Redesign] = None, scaffold: Optional[Scaffold] = None, sequence_rules: Optional[SequenceRules] = None,
               solver: Optional[Solver] = None, guidance: Optional[Guidance] = None):
        """``guidance`` (guidance.Guidance, keyword only): distance restraints and clash repulsion, evaluated on every step's
        clean-structure estimate and added to the predicted noise (``ReverseDiffusion``).
        ``solver`` (solver.Solver, keyword only): visit K chosen levels instead of all ``num_steps`` -- strided ancestral sampling or
        DDIM, K network evaluations per sample (``ReverseDiffusion``); a repeat under fp32 runs the same solver.
        ``scaffold`` (conditioning.Scaffold, keyword only): keep rows of the complex where the input structure has them and / or
        start from the noised input (``ReverseDiffusion``); the positions then come back in the INPUT's frame.  ``sequence_rules``
        (sequence.SequenceRules, keyword only): the classes the ruled residues may take and the bias on their logits, applied to the
        sequence state after every step and to the returned logits (``ReverseDiffusion``)."""
        self.check_widths()
        redesign = self._redesign_spec(redesign)        # deterministic: the fp32 repeat below prepares the same mask, nothing memoised
        cond = {} if self._scaffold_spec(scaffold) is None else {"scaffold": scaffold}
        if self._rules_spec(sequence_rules) is not None:         # deterministic too: the repeat prepares the same tables
            cond["sequence_rules"] = sequence_rules
        if self._solver_spec(solver, scaffold) is not None:     # an immutable value: the repeat computes the same tables
            cond["solver"] = solver
        if self._guidance_spec(guidance, solver) is not None:   # an immutable value too
            cond["guidance"] = guidance
        if sources is None:
            sources = self._sources(batch["atom_mask"].shape[0], batch_idx)
        if self.training_mode and mask_draws is None:
            mask_draws = self._mask_draws()             # ONE draw per call (memoised): the fp32 repeat below prepares the same mask
        # the keyed generators are consumed by a loop: remember where they stood so that a repeat draws the same noise
        states = [s.g.get_state() if hasattr(s, "g") else None for s in sources]
        with _lib.arithmetic(self.arithmetic):
            loop = ReverseDiffusion(self, batch, sources, mask_draws, redesign, **cond)
            loop.run()
            cur = _lib.arith()
            if self.nonfinite_policy == "off" or loop.finite():
                return loop.result()
        if cur == 1 and self.nonfinite_policy == "fp32":
            import warnings
            warnings.warn(f"sample: inf / NaN after {loop.steps_done} denoising steps under split-16 arithmetic (an operand beyond the "
                          "fp16 range: include/prd_hip.h, OPERAND RANGE); running the call again under PRD_ARITH_FP32 and keeping fp32 "
                          "for this model", RuntimeWarning, stacklevel=2)
            if any(st is None for st in states):
                raise _lib.NonFiniteError("sample: non-finite under split-16 arithmetic and the noise sources cannot be rewound")
            for s, st in zip(sources, states):
                s.g.set_state(st)
            self.arith_fallbacks += 1
            self.arithmetic = "fp32"
            with _lib.arithmetic("fp32"):
                loop = ReverseDiffusion(self, batch, sources, mask_draws, redesign, **cond)
                loop.run()
                if loop.finite():
                    return loop.result()
            cur = 0
        raise _lib.NonFiniteError(f"sample: inf / NaN coordinates or logits under {_lib.ARITH_NAMES[cur]} arithmetic"
                                  + (" (the fp32 repeat of a non-finite split-16 call)" if self.arith_fallbacks and cur == 0 else "")
                                  + (": outside the operand range of the split arithmetic (include/prd_hip.h); set model.arithmetic = 'fp32' "
                                     "or nonfinite_policy = 'fp32'" if cur == 1 else ": the weights / inputs themselves produce inf or NaN"))


def update_noise_rows(solver: Optional[Solver], T: int) -> int:
    """Update-noise tensors [N,3] a loop draws per source after z_T and seq_T: T - 1 without a solver, K - 1 under a stochastic one,
    none under a deterministic one."""
    if solver is None:
        return T - 1
    return solver.K - 1 if solver.stochastic else 0


def conditioning_noise_rows(solver: Optional[Solver], T: int, start: Optional[int]) -> int:
    """Conditioning-noise tensors [N,3] a scaffold adds per source, after every other draw: one per level the loop visits"""
    if solver is not None:
        return solver.K
    return (T - 1 if start is None else start) + 1


def draw_loop_noise(sources, N: int, rows: int):
    """(z_T [b,N,3], seq_T [b,N,21], update noise [rows,b,N,3] or None for rows = 0) from each sample's keyed source, in the
    reference's per-sample order: z_T, seq_T, then the update tensors in the order the loop consumes them.  Host only."""
    z0 = torch.stack([s.randn(N, 3) for s in sources])
    s0 = torch.stack([s.randn(N, NUM_RESIDUE_CLASSES) for s in sources])
    noise = torch.stack([torch.stack([s.randn(N, 3) for _ in range(rows)]) for s in sources], dim=1) if rows > 0 else None
    return z0, s0, noise


def draw_conditioning_noise(sources, N: int, rows: int) -> torch.Tensor:
    """[rows,b,N,3]: per source ``rows`` tensors for the visited levels, highest level first.  Host only."""
    return torch.stack([torch.stack([s.randn(N, 3) for _ in range(rows)]) for s in sources], dim=1)


class ReverseDiffusion:
    """State and driver of one ``sample()`` call (reference model.py:377-422) on one GPU.

    Everything the loop needs is resident in HBM before the first step: the step-invariant
    embeddings, the complete noise table ``[T-1, b, N, 3]`` (drawn on the host from the keyed
    generators, in the reference's per-sample order) and the per-step scalar
    table.  ``z``, ``seq_t`` and the step counter ``t`` live on the device and are advanced by the
    kernels themselves, so ONE captured hipGraph of a whole step (network forward + reverse update)
    is replayed for every remaining step: no per-step host work and no ``(t == 0).all()``
    device->host sync (model.py:415).

    ``scaffold`` (conditioning.Scaffold; beyond the reference): replacement conditioning in the centred frame.  The
    rows K the spec keeps never follow the reverse update: the state entering the step with counter l has
    ``z[K] = A[l] x0c[K] + S[l] eps_l[K]`` (x0c: ``batch["x"]`` minus its masked mean, A / S: the model's sqrt_alphas_cumprod /
    sqrt_one_minus_alphas_cumprod, eps_l: mean-free noise of its own per level), and ``z[K] = x0c[K]`` after the last step; one
    launch of prd_condition_rows after every boundary, inside the captured graph, does it (and, with ``sequence=True``, puts the known
    residues' one-hot rows back, followed by one prd_single_init under the fused boundary).  ``start = L`` begins at level L from the
    noised input and runs L + 1 steps on the noise rows the uninterrupted loop consumes from there.  ``result()`` is then in the
    input's frame.  The conditioning noise -- per source L + 1 tensors [N,3] for the levels L .. 0 (L = T - 1 without ``start``), drawn
    AFTER everything an unconditioned loop draws, so the other draws are what they were -- is a second device table
    ``[L+1, b, N, 3]``: with a scaffold the loop's noise memory doubles.

    ``sequence_rules`` (sequence.SequenceRules; beyond the reference): the bias table goes up once and the ruled rows
    (the design region, or every residue) are built once.  After every boundary, inside the captured graph, one launch of
    prd_sequence_constrain rewrites the ruled rows of ``seq_t`` from the logits of that step: ``2 p - 1`` with p the softmax of
    ``seq_pred + bias`` over the allowed classes, exactly -1 at a banned class; under the fused boundary one prd_single_init then
    rebuilds the coming step's single input.  With ``Scaffold(sequence=True)`` as well the order is constrain, hold, one
    prd_single_init: a held row wins.  A spec without any ban or bias (``inert``) rules no row by construction and launches nothing.
    The initial ``seq_t`` is noise on the design rows, as the reference initialises it, and stays as it is.  ``result()`` returns the
    logits with the rules applied on the ruled rows.

    ``solver`` (solver.Solver; beyond the reference): the loop visits the K levels ``tau_{K-1} > ... > tau_0`` the
    spec chooses instead of all T.  A device counter ``k`` runs from K - 1 down to 0 beside ``t``, which holds the level itself;
    ``steps_done``, ``run()``, ``reset()`` and ``restart(step, ...)`` count solver steps in [0, K).  The boundary of every step is ONE
    launch of prd_solver_boundary (include/prd_solver.h), which indexes the level table [K] and the coefficient table [K,8]
    (``Solver.tables``: float64 on the host, rounded once) by the counter; it has no un-fused form, so PRD_FUSED_BOUNDARY does not
    apply.  One captured graph serves every step, and a replayed step has the launches it had.  A stochastic solver draws K - 1 update
    tensors per source where the T - 1 of the full loop sit (the table is [K-1, b, N, 3], row K - 1 - k consumed at counter k > 0); a
    deterministic one (``Solver.ddim(K)``) draws none and uploads no table.  ``x0_hat`` [b,N,3] holds the clean-structure estimate of
    the last step, centred and in nanometres.  With a scaffold the kept rows are noised to the level that comes NEXT: the level and
    conditioning-noise tables are compressed to the visited levels ([K,2], [K,b,N,3]: K conditioning draws per source) and
    prd_condition_rows is handed the counter; ``start = L`` spreads the K levels over [L .. 0].  ``Solver.ancestral(T)`` is the loop
    without a solver, bit for bit.

    A multistep solver of order 2 or 3 (``Solver.multistep``, ``Solver.dpmpp_2m``) is the deterministic ddim loop on its
    levels plus ONE launch of prd_multistep_correct (include/prd_multistep.h) directly after every boundary, inside the captured graph:
    it adds the step's gains (``Solver.gain_table`` [K,4]: float64 on the host, rounded once) times the differences between ``x0_hat``
    and the estimates of the previous one or two steps to ``z``, then pushes ``x0_hat`` onto the history ``x0_hist`` [2,b,N,3].  ``first``
    [b] holds the counter of the first step run since ``reset()`` / ``restart()``, which both set with a ``fill_``: the history of another
    trajectory is never used, and the order builds up again over two steps.  A replayed step has one launch more than under
    ``Solver.ddim``; the kept rows of a scaffold are overwritten after the correction.  With guidance the history holds the guided
    estimate, which is what the boundary writes.  Order 1 allocates, uploads and launches nothing: it is the ddim loop, bit for bit.

    ``guidance`` (guidance.Guidance; beyond the reference): between the network and the boundary of every step ONE
    launch of prd_guide_eps (include/prd_guide.h) evaluates the clash and restraint energy on the step's clean-structure estimate and
    writes ``eps_raw + lam dE/dx0`` (capped per position) into a loop-owned buffer, which the boundary then receives in place of the
    coordinate head's output.  The table {q, r, lam, cap} per counter (``Guidance.tables``: float64 on the host, rounded once; the rows
    of the visited levels under a solver), the restraint lists and the clash floors go up once; the classes and the bond exclusions are
    built on the device.  ``guidance_energy`` [b,N,2] holds every row's share of the clash and restraint energy at the last step's
    estimate.  A replayed step has one launch more.  With a scaffold the kept rows are overwritten after the boundary as before: forces
    on them are harmless and are not special-cased.  An ``inert`` spec launches nothing and uploads nothing.  A restraint must name rows
    of the batch; rows beyond a sample's valid ones hold no structure, and ``pipeline.generate_samples`` refuses them on the host data."""

    def __init__(self, model: "ProteinReDiffModel", batch, sources: Optional[Sequence] = None, mask_draws: Optional[MaskDraws] = None,
                 redesign: Optional[Redesign] = None, scaffold: Optional[Scaffold] = None, sequence_rules: Optional[SequenceRules] = None,
                 solver: Optional[Solver] = None, guidance: Optional[Guidance] = None):
        m = self.model = model
        self.scaffold = scaffold = m._scaffold_spec(scaffold)
        self.sequence_rules = sequence_rules = m._rules_spec(sequence_rules)
        self.solver = solver = m._solver_spec(solver, scaffold)
        self.guidance = guidance = m._guidance_spec(guidance, solver)
        if guidance is not None:
            guidance.check_rows(batch["atom_mask"].shape[1], "the batch's rows")
            if guidance.inert:
                guidance = None                 # nothing can ever be added: nothing is uploaded, nothing is launched
        if not m.setup_schedule:
            m.run_setup_schedule()
            m.setup_schedule = True
        dev = m.device
        b, N = batch["atom_mask"].shape
        if sources is None:
            sources = m._sources(b)
        self.batch = batch = m.prepare_batch(batch, sources=sources, mask_draws=mask_draws, redesign=redesign)
        self.mask = batch["residue_and_atom_mask"].contiguous()
        self.rm = batch["residue_mask"].contiguous()
        self.T = T = m.num_steps
        self.K = T                              # steps_done of a finished loop: T, or the K of a solver
        if solver is not None:
            # host arithmetic only: the full-length special case recomputes the rows of m._coef as run_setup_schedule does (equal bits)
            # instead of reading them back from the device
            levels, coef = solver.tables(T, m.diffusion_schedule, scaffold.start if scaffold is not None else None)
            self._levels = levels.tolist()      # host copy: restart() and reset() look levels up without reading the device
            self.K = len(self._levels)
        z0, s0, noise = draw_loop_noise(sources, N, update_noise_rows(solver, T))
        if noise is None and solver is None:
            noise = torch.zeros(1, b, N, 3)
        # with a scaffold, sequence rules, a solver or guidance the tables go up from pinned staging, ordered on the current stream, so that such
        # a loop is set up without a host synchronisation; without any of them the uploads are the pageable copies they were
        pinned = (scaffold is not None or sequence_rules is not None or solver is not None or guidance is not None) and dev.type == "cuda"
        up = self._upload = (lambda x: x.pin_memory().to(dev, non_blocking=True)) if pinned else (lambda x: x.to(dev))
        self.noise = up(noise).contiguous() if noise is not None else None      # [T-1, b, N, 3]; a solver: [K-1, b, N, 3] or None
        self.z = ops.remove_mean(up(z0).contiguous(), self.mask)
        seq_t = ops.remove_mean(up(s0).contiguous(), self.rm)
        self.seq_t = (batch["residue_extra_mask"].unsqueeze(-1) * batch["residue_one_hot"]
                      + batch["residue_inv_extra_mask"].unsqueeze(-1) * seq_t).contiguous()
        self.static = m._static_inputs(batch)
        self._first = (T - 1, 0)                # (counter, steps done) of a fresh loop
        self.cond = None                        # the arguments of condition_rows_ after every boundary (None: nothing to hold)
        self.rules = None                       # (bias table [1 or b,N,21], ruled rows [b,N]) of constrain_rows_ after every boundary
        if sequence_rules is not None:          # an inert spec (no ban, no bias) rules no row by construction: nothing is launched for it
            if not sequence_rules.inert:
                self.rules = (sequence_rules.table(batch), sequence_rules.rows(batch))
            batch[RULES_KEY] = self.rules[1] if self.rules is not None else torch.zeros_like(self.rm)
        self.t = torch.full((b,), T - 1, dtype=torch.int64, device=dev)
        self.k = self.x0_hat = None
        if solver is not None:                  # the counter beside the level, the two tables, the estimate of the last step
            self._first = (self.K - 1, 0)
            self.t.fill_(self._levels[-1])
            self.k = torch.full((b,), self.K - 1, dtype=torch.int64, device=dev)
            self.levels, self.coef = up(levels), up(coef)
            self.x0_hat = torch.zeros(b, N, 3, dtype=torch.float32, device=dev)
        self.gain = self.x0_hist = self.first = None    # a multistep solver of order 2 or 3: the gains, the last two estimates, the first counter
        if solver is not None and solver.corrected:
            self.gain = up(solver.gain_table(T, m.diffusion_schedule, scaffold.start if scaffold is not None else None))
            self.x0_hist = torch.zeros(2, b, N, 3, dtype=torch.float32, device=dev)
            self.first = torch.full((b,), self.K - 1, dtype=torch.int64, device=dev)
        self.guide = self.guidance_energy = None        # the step-invariant arguments of guide_eps_ (None: no launch), its e_out
        if guidance is not None:
            self.guide = guidance.terms(batch, up)
            self.guide["table"] = up(guidance.tables(T, m.diffusion_schedule, self._levels if solver is not None else None))
            self._eps_guided = torch.empty(b, N, 3, dtype=torch.float32, device=dev)
            self.guidance_energy = torch.zeros(b, N, 2, dtype=torch.float32, device=dev)
        if scaffold is not None:
            self._condition(scaffold, sources, b, N, dev)
        self._init = (self.z.clone(), self.seq_t.clone())
        self.steps_done = self._first[1]
        self.graph = None
        self.seq_pred = None
        # inputs of the coming step that the previous step's boundary kernel prepares (single, time embedding)
        import os
        # time_dim > 512: the fused boundary has no room for the time features; the separate launches serve any width.  Under a solver
        # the boundary is always the one launch of prd_solver_boundary (no un-fused form; _solver_spec refused a wider time_dim)
        self.fused_boundary = solver is not None or os.environ.get("PRD_FUSED_BOUNDARY", "1") != "0" and ops.step_boundary_fusable(m.time_dim)
        self.sync = torch.zeros(2, dtype=torch.int32, device=dev)     # [0] arrival counter, [1] sticky non-finite flag (prd_step_boundary)
        self._seq_pred_buf = None               # logits of the last step (written by the step-boundary kernel)
        self.single_in, self.eb_in = m._step_inputs(self.static, self.seq_t, self.rm, self.t)

    def _condition(self, scaffold: Scaffold, sources, b, N, dev):
        """Set-up of a conditioned loop: x0c, centre, the kept rows K, the level table [T,2], the conditioning noise [L+1,b,N,3] (drawn
        here, after every draw of an unconditioned loop; mean-removed once), the initial state and the first counter.  No host sync."""
        m, batch, T = self.model, self.batch, self.T
        L = T - 1 if scaffold.start is None else scaffold.start
        x0 = batch["x"].to(torch.float32).contiguous()
        self.x0c = ops.remove_mean(x0, self.mask)
        valid = self.mask.unsqueeze(-1)
        self.centre = (valid * x0).sum(dim=1, keepdim=True) / valid.sum(dim=1, keepdim=True)       # [b,1,3]: the masked mean
        self._offset = valid * self.centre                                                         # what result() adds: valid rows only
        self.keep = scaffold.rows(batch)                                                           # K [b,N] or None
        batch[SCAFFOLD_KEY] = self.keep if self.keep is not None else torch.zeros_like(self.mask)
        self.level = level_table({k: getattr(m, k) for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")})
        # one conditioning draw per level the loop visits, highest first: L + 1 without a solver, K with one -- whose tables are
        # compressed to the visited levels and indexed by the counter (row k: level tau_k; rows picked, no arithmetic)
        rows = conditioning_noise_rows(self.solver, T, scaffold.start)
        if self.solver is not None:
            self.level = self.level[self.levels].contiguous()
        draws = draw_conditioning_noise(sources, N, rows)                                              # [rows,b,N,3]: levels L .. 0
        table = self._upload(draws.flip(0).contiguous())                                               # indexed by level / by counter
        self.cond_noise = ops.remove_mean(table.view(rows * b, N, 3), self.mask.repeat(rows, 1)).view(rows, b, N, 3)
        seq = dict(seq0=batch["residue_one_hot"].to(torch.float32).contiguous(),
                   keep_seq=batch["residue_extra_mask"].to(torch.float32).contiguous()) if scaffold.sequence else {}
        held = dict(x0c=self.x0c, noise=self.cond_noise, level=self.level)
        if self.solver is None:
            self.t.fill_(L)
            self._first = (L, T - 1 - L)
        # the initial state: with ``start`` every valid row is the noised input, otherwise the kept ones
        first = self.mask if scaffold.start is not None else self.keep
        if first is not None or seq:
            condition_rows_(self.z, self.seq_t, self._counter, keep_z=first, **(held if first is not None else {}), **seq)
        if self.keep is not None or seq:
            self.cond = dict(keep_z=self.keep, **(held if self.keep is not None else {}), **seq)

    @property
    def _counter(self):
        """what indexes the tables of prd_condition_rows: the level itself, or under a solver the counter over the visited levels"""
        return self.k if self.solver is not None else self.t

    def _hold_rows(self, seq_pred):
        """After a boundary: the ruled rows of seq_t retaken under the sequence rules from the step's logits ``seq_pred``
        (sequence.constrain_rows_), then the kept rows back onto the noised input at the counter the boundary left and, with the clamp,
        onto the known sequence (conditioning.condition_rows_) -- a held row wins.  If either rewrote seq_t under the fused boundary,
        ONE prd_single_init builds the coming step's single input from it."""
        clamp = self.cond is not None and self.cond.get("keep_seq") is not None
        if self.rules is not None:
            constrain_rows_(self.seq_t, seq_pred, *self.rules)
        if self.cond is not None:
            condition_rows_(self.z, self.seq_t, self._counter, **self.cond)
        if self.fused_boundary and (clamp or self.rules is not None):
            ops.single_init(self.static["single"], self.seq_t, self.rm, self.model.embed_residue_type[1].weight, out=self.single_in)

    def _guide(self, eps_raw):
        """Between the network and the boundary: the guided predicted noise in the loop's own buffer (prd_guide_eps, indexed by the
        counter the boundary is about to consume), or ``eps_raw`` itself without guidance"""
        if self.guide is None:
            return eps_raw
        g = self.guide
        guide_eps_(self.z, eps_raw.contiguous(), self._eps_guided, self.mask, self._counter, g["table"], g["cls"], g["floors"], g["wclash"],
                   g["exclude"], g["csr"], self.guidance_energy)
        return self._eps_guided

    def _refresh_step_inputs(self):
        single, eb = self.model._step_inputs(self.static, self.seq_t, self.rm, self.t)
        self.single_in.copy_(single)
        self.eb_in.copy_(eb)

    def _set_counter(self, counter: int):
        """every sample at ``counter``: the level itself, or under a solver the counter and the level it stands for (host values)"""
        if self.solver is None:
            self.t.fill_(counter)
        else:
            self.k.fill_(counter)
            self.t.fill_(self._levels[counter])
            if self.first is not None:          # the history belongs to the trajectory that ends here: the order builds up again
                self.first.fill_(counter)

    def reset(self):
        """Back to step T-1 with the same initial noise (bench / repeated runs)."""
        self.z.copy_(self._init[0])
        self.seq_t.copy_(self._init[1])
        self._set_counter(self._first[0])
        self.steps_done = self._first[1]
        self._refresh_step_inputs()

    def restart(self, step: int, z: torch.Tensor, seq_t: torch.Tensor):
        """Continue from a given state: ``z`` / ``seq_t`` are the tensors ENTERING denoising step number ``step`` (0 = the
        first, t = T-1).  The pre-drawn noise table is indexed by the step counter, so the continuation consumes exactly the
        noise the uninterrupted loop would (checkpointed sampling; segment-wise parity tests)."""
        if not 0 <= step < self.K:
            raise ValueError(f"step must be in [0, {self.K}), got {step}")
        self.z.copy_(z.to(self.z.device))
        self.seq_t.copy_(seq_t.to(self.seq_t.device))
        self._set_counter(self.K - 1 - step)
        self.steps_done = step
        if self.cond is not None:               # the kept rows of the given state, at its level
            condition_rows_(self.z, self.seq_t, self._counter, **self.cond)
        self._refresh_step_inputs()

    def _enqueue_step(self):
        """Network forward on the inputs the previous boundary prepared, then ONE step-boundary launch: remove_mean, reverse
        update, t <- t - 1 and the next step's single / time-embedding inputs (ops.step_boundary_)."""
        m = self.model
        if self.solver is not None:             # the same step with prd_solver_boundary as its one boundary launch
            eps_raw, seq_h = m._network(self.batch, self.z, self.seq_t, self.mask, self.t, static=self.static,
                                        step_inputs=(self.single_in, self.eb_in), raw_noise=True, defer_seq_head=True)
            if self._seq_pred_buf is None:
                self._seq_pred_buf = torch.empty(*self.seq_t.shape, device=self.seq_t.device, dtype=torch.float32)
            eps_raw = self._guide(eps_raw)
            solver_boundary_(self.z, self.seq_t, self.k, self.t, eps_raw, self._seq_pred_buf, self.noise, self.mask, self.levels, self.coef,
                             self.T, self.single_in, self.static["single"], self.rm, m.embed_residue_type[1].weight,
                             self.eb_in, m.embed_beta[0].weight, m.embed_beta[1].weight, self.sync, x0_out=self.x0_hat,
                             seq_h=seq_h, w_seq=m.seq_mlp[3].weight)
            if self.gain is not None:           # the higher-order correction on the counter the boundary left, and the push of x0_hat
                multistep_correct_(self.z, self.x0_hat, self.x0_hist, self.k, self.first, self.gain)
            if self.cond is not None or self.rules is not None:
                self._hold_rows(self._seq_pred_buf)
            return self._seq_pred_buf
        if not self.fused_boundary:             # the four separate launches (kept for A/B measurements: PRD_FUSED_BOUNDARY=0)
            noise_pred, seq_pred = m._network(self.batch, self.z, self.seq_t, self.mask, self.t, static=self.static)
            ops.reverse_update_(self.z, self.seq_t, self.t, noise_pred, seq_pred, self.noise, self.mask, m._coef, self.T)
            if self.cond is not None or self.rules is not None:
                self._hold_rows(seq_pred.contiguous())
            return seq_pred
        eps_raw, seq_h = m._network(self.batch, self.z, self.seq_t, self.mask, self.t, static=self.static,
                                    step_inputs=(self.single_in, self.eb_in), raw_noise=True, defer_seq_head=True)
        if self._seq_pred_buf is None:
            self._seq_pred_buf = torch.empty(*self.seq_t.shape, device=self.seq_t.device, dtype=torch.float32)
        eps_raw = self._guide(eps_raw)
        ops.step_boundary_(self.z, self.seq_t, self.t, eps_raw, self._seq_pred_buf, self.noise, self.mask, m._coef, self.T,
                           self.single_in, self.static["single"], self.rm, m.embed_residue_type[1].weight,
                           self.eb_in, m.embed_beta[0].weight, m.embed_beta[1].weight, self.sync,
                           seq_h=seq_h, w_seq=m.seq_mlp[3].weight)
        if self.cond is not None or self.rules is not None:
            self._hold_rows(self._seq_pred_buf)
        return self._seq_pred_buf

    @torch.inference_mode()
    def step(self):
        """One denoising step: network forward + reverse update (asynchronous)."""
        if self.steps_done >= self.K:
            raise RuntimeError("all num_steps denoising steps already done; call reset()" if self.solver is None else
                               f"all {self.K} solver steps already done; call reset()")
        if self.graph is not None:
            self.graph.replay()
        elif self.model.use_hip_graph and self.steps_done >= 1 + self._first[1]:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.seq_pred = self._enqueue_step()      # capture only; the replay below executes it
            self.graph.replay()
        else:
            self.seq_pred = self._enqueue_step()          # first step eager: warms every kernel up
        self.steps_done += 1

    def run(self):
        while self.steps_done < self.K:
            self.step()

    def finite(self) -> bool:
        """False when the loop produced inf / NaN: the sticky flag the step-boundary kernel keeps (any step, prd_hip.h) or'ed with a
        check of the current state and logits (covers the un-fused boundary and direct step() use).  ONE host read per call --
        after the loop, never inside it."""
        bad = self.sync[1] != 0
        bad = bad | ~torch.isfinite(self.z).all()
        if self.seq_pred is not None:
            bad = bad | ~torch.isfinite(self.seq_pred).all()
        return not bool(bad)

    def result(self):
        """(positions in Angstrom, residue-masked logits) as in model.py:421-422.  With a scaffold the valid rows come back in the
        input's frame, ``10 (z + centre)``: the kept rows at the input's own coordinates, the rebuilt ones beside them.  With sequence
        rules the logits of the ruled rows are ``seq_pred + bias`` where allowed and exactly BANNED where banned, so that a host argmax
        (pipeline.predict_seq) honours them: one elementwise expression here, after the loop."""
        logits = self.rm.unsqueeze(-1) * self.seq_pred
        if self.rules is not None:              # the ruled rows are residues: the mask above left them as they were
            logits = self.sequence_rules.apply(logits, *self.rules)
        if self.scaffold is not None:
            return 10.0 * (self.z + self._offset), logits
        return 10.0 * self.z, logits
