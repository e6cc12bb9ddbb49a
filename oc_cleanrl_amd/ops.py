"""torch-facing wrappers of the HIP kernels (libocppo_hip.so).

Every function takes CUDA (HIP) tensors, validates shapes/dtypes/devices on the host before any
launch, and launches on the current torch stream of the tensors' device, so everything here is
asynchronous and capturable into a torch.cuda.CUDAGraph (hipGraph). There is no CPU fallback: a
CPU tensor is an error.

Reference lines replaced are cited per function (paths relative to the reference checkout).
"""
from __future__ import annotations

import ctypes
import functools
import math

import torch

from . import _lib
from ._lib import (OCPPO_BF16, OCPPO_F32, OCPPO_NET_CHANNELS_LAST, OCPPO_NET_SCALE_255, OCPPO_U8,
                   STAT_NAMES, call)

_DTYPE_CODE = {torch.float32: OCPPO_F32, torch.bfloat16: OCPPO_BF16, torch.uint8: OCPPO_U8}


def _check(t: torch.Tensor, name: str, dtype: torch.dtype | None = None, device=None,
           numel: int | None = None) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise ValueError(f"{name}: HIP kernels need a GPU tensor, got device {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name}: has {t.numel()} elements, expected {numel}")
    return t.data_ptr()


def _opt(t, *a, **k) -> int | None:
    return None if t is None else _check(t, *a, **k)


def _net_obs(net_obs, N: int, W: int, D: int, device):
    """(pointer, layout) of a rollout network-input buffer: a contiguous [N, W, ...] f32 tensor
    (layout 0) or a channels_last [N, W, H, X] one (layout OCPPO_NET_CHANNELS_LAST: memory
    [N, H, X, W], the NHWC input of a channels_last NatureCNN)."""
    if net_obs is None:
        return None, 0
    if net_obs.is_contiguous():
        return _check(net_obs, "net_obs", torch.float32, device, N * W * D), 0
    if net_obs.dim() == 4 and net_obs.is_contiguous(memory_format=torch.channels_last) and \
            tuple(net_obs.shape[:2]) == (N, W) and net_obs[0, 0].numel() == D:
        if net_obs.dtype != torch.float32 or net_obs.device != device:
            raise ValueError(f"net_obs: expected float32 on {device}")
        return net_obs.data_ptr(), OCPPO_NET_CHANNELS_LAST
    raise ValueError("net_obs must be contiguous [N, W, ...] or channels_last [N, W, H, X]")


# Optional per-launch timer for launch sites inside autograd (the trainer's KernelTimer when
# kernel timing is on): timed(name, fn) runs fn and lets the timer keep its first eager launch.
TIMER = None


def timed(name: str, fn):
    return TIMER.bracket(name, fn) if TIMER is not None else fn()


# gemm_x6 launches issued with pre-split weight planes, by (M, N, K): host-side bookkeeping at
# issue time (under capture: once per captured launch), so tests can see that the planes a
# WeightPlanes refresh writes are actually read
PLANE_USES: dict = {}


def _note_planes(b_planes, M: int, N: int, K: int):
    if b_planes is not None:
        PLANE_USES[(M, N, K)] = PLANE_USES.get((M, N, K), 0) + 1


def _stream(device: torch.device) -> int:
    if device.type != "cuda":
        raise ValueError(f"HIP kernels need GPU tensors, got device {device} (no CPU fallback)")
    return torch.cuda.current_stream(device).cuda_stream


# Every per-shape workspace of this module (split-K partials, ticket and flag words, index
# tables), by (tag, device, key). A (tag, device, key) is allocated at most once per process and
# never freed or resized: captured hipGraphs hold the pointer. The launches of one stream share a
# buffer (they run one after another); trainers on different streams share it too.
_PERSISTENT: dict = {}


def _persistent(tag: str, dev, key, make):
    """The buffer `make()` returned the first time (tag, dev, key) was asked for. tag: the owning
    entry point's name, so two entry points never share one; dev: any spelling of a device (the
    key holds it with an explicit index: "cuda" and "cuda:0" are one GPU)."""
    buf = _PERSISTENT.get((tag, dev, key))  # a tensor's .device is in the key's form already
    if buf is None:
        dev = torch.device(dev)
        if dev.index is None:
            dev = torch.device(dev.type, torch.cuda.current_device() if dev.type == "cuda" else 0)
        buf = _PERSISTENT.get((tag, dev, key))
        if buf is None:
            buf = _PERSISTENT[(tag, dev, key)] = make()
    return buf


# ---------------------------------------------------------------------------------------------
# GAE (ppo_atari_oc.py:533-547)
# ---------------------------------------------------------------------------------------------
def gae(rewards, values, dones, next_value, next_done, gamma: float, gae_lambda: float,
        advantages=None, returns=None, logprobs=None, actions=None, records=None):
    """Advantages and returns of one rollout; [T, N] f32 in, ([T, N], [T, N]) out.

    Bit-identical to the reference loop. `next_value` may be [N] or [1, N] (as produced by
    `agent.get_value(next_obs).reshape(1, -1)`). records (with logprobs [T, N] f32 and actions
    [T, N] i64 in [0, 2^31)): also write each sample's 16-B record (sample_records) for
    minibatch_prepare(records=...).
    """
    if rewards.dim() != 2:
        raise ValueError(f"rewards must be [T, N], got {tuple(rewards.shape)}")
    T, N = rewards.shape
    dev = rewards.device
    f = torch.float32
    if advantages is None:
        advantages = torch.empty_like(rewards)
    if returns is None:
        returns = torch.empty_like(rewards)
    args = (_check(rewards, "rewards", f, dev),
            _check(values, "values", f, dev, T * N), _check(dones, "dones", f, dev, T * N),
            _check(next_value, "next_value", f, dev, N), _check(next_done, "next_done", f, dev, N),
            T, N, float(gamma), float(gae_lambda), _check(advantages, "advantages", f, dev, T * N),
            _check(returns, "returns", f, dev, T * N))
    if records is None:
        call("ocppo_gae", _stream(dev), *args)
    else:
        call("ocppo_gae_records", _stream(dev), *args,
             _check(logprobs, "logprobs", f, dev, T * N),
             _check(actions, "actions", torch.int64, dev, T * N),
             _check(records, "records", torch.int32, dev, 4 * T * N))
    return advantages, returns


def sample_records(B: int, device):
    """[B] x 16-B per-sample records (ocppo.h OcppoSampleRecord) as an int32 [B, 4] tensor."""
    return torch.zeros((B, 4), dtype=torch.int32, device=device)


# ---------------------------------------------------------------------------------------------
# minibatch advantage statistics (ppo_atari_oc.py:577-579)
# ---------------------------------------------------------------------------------------------
def minibatch_adv_stats(b_advantages, perm, minibatch_size: int, out=None):
    """(mean, unbiased std) of b_advantages over each minibatch of `perm` → [num_mb, 2]."""
    dev = b_advantages.device
    if perm.numel() % minibatch_size:
        raise ValueError("perm length must be a multiple of minibatch_size")
    num_mb = perm.numel() // minibatch_size
    if out is None:
        out = torch.empty((num_mb, 2), dtype=torch.float32, device=dev)
    call("ocppo_minibatch_adv_stats", _stream(dev),
         _check(b_advantages, "b_advantages", torch.float32, dev),
         _check(perm, "perm", torch.int64, dev), minibatch_size, num_mb,
         _check(out, "out", torch.float32, dev, 2 * num_mb))
    return out


def minibatch_prepare(perm, minibatch_size: int, b_actions, b_logprobs, b_advantages, b_returns,
                      b_values, out: dict | None = None, with_stats: bool = True, records=None):
    """Gather every minibatch's per-sample arrays into minibatch order (+ adv stats).
    records: the 16-B per-sample records of gae(records=...) gathered instead of the five b_*
    arrays (then only their sizes are read; bitwise the same outputs).

    Returns dict(actions, logprobs, advantages, returns, values: [num_mb*M], adv_stats [num_mb,2])."""
    dev = perm.device
    M = minibatch_size
    n = perm.numel()
    if n % M:
        raise ValueError("perm length must be a multiple of minibatch_size")
    num_mb = n // M
    B = b_logprobs.numel()
    f = torch.float32
    if records is not None:
        if out is None:
            out = {"actions": torch.empty(n, dtype=torch.int64, device=dev),
                   **{k: torch.empty(n, dtype=f, device=dev)
                      for k in ("logprobs", "advantages", "returns", "values")},
                   "adv_stats": torch.empty((num_mb, 2), dtype=f, device=dev)}
        call("ocppo_minibatch_prepare_records", _stream(dev),
             _check(perm, "perm", torch.int64, dev), M, num_mb,
             _check(records, "records", torch.int32, dev, 4 * B),
             _check(out["actions"], "mb_actions", torch.int64, dev, n),
             _check(out["logprobs"], "mb_logprobs", f, dev, n),
             _check(out["advantages"], "mb_advantages", f, dev, n),
             _check(out["returns"], "mb_returns", f, dev, n),
             _check(out["values"], "mb_values", f, dev, n),
             _check(out["adv_stats"], "adv_stats", f, dev, 2 * num_mb) if with_stats else None)
        return out
    if out is None:
        out = {"actions": torch.empty(n, dtype=torch.int64, device=dev),
               **{k: torch.empty(n, dtype=f, device=dev)
                  for k in ("logprobs", "advantages", "returns", "values")},
               "adv_stats": torch.empty((num_mb, 2), dtype=f, device=dev)}
    call("ocppo_minibatch_prepare", _stream(dev), _check(perm, "perm", torch.int64, dev), M,
         num_mb, _check(b_actions, "b_actions", torch.int64, dev, B),
         _check(b_logprobs, "b_logprobs", f, dev, B), _check(b_advantages, "b_advantages", f, dev, B),
         _check(b_returns, "b_returns", f, dev, B), _check(b_values, "b_values", f, dev, B),
         _check(out["actions"], "mb_actions", torch.int64, dev, n),
         _check(out["logprobs"], "mb_logprobs", f, dev, n),
         _check(out["advantages"], "mb_advantages", f, dev, n),
         _check(out["returns"], "mb_returns", f, dev, n),
         _check(out["values"], "mb_values", f, dev, n),
         _check(out["adv_stats"], "adv_stats", f, dev, 2 * num_mb) if with_stats else None)
    return out


# ---------------------------------------------------------------------------------------------
# fused PPO loss (ppo_atari_oc.py:566-602 from the network outputs on)
# ---------------------------------------------------------------------------------------------
class LossWorkspace:
    """Device scratch for ppo_loss_fwd_bwd (zeroed once; the kernel re-arms its ticket)."""

    def __init__(self, M: int, A: int, device):
        n = _lib.LIB.ocppo_ppo_loss_workspace_bytes(M, A)
        self.nbytes = int(n)
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.M, self.A = M, A


def ppo_loss_fwd_bwd(logits, new_value, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                     *, mb_inds=None, adv_stats=None, clip_coef: float, ent_coef: float,
                     vf_coef: float, norm_adv: bool, clip_vloss: bool, dlogits=None, dvalue=None,
                     stats=None, workspace: LossWorkspace | None = None):
    """One launch: loss statistics [9] plus dLoss/dlogits [M, A] and dLoss/dvalue [M].

    `b_*` are the flattened batch arrays (b_actions int64); `mb_inds` selects the minibatch
    (None = the b_* arrays are already the minibatch). Returns (stats, dlogits, dvalue); stats
    layout = _lib.STAT_NAMES.
    """
    if logits.dim() != 2:
        raise ValueError(f"logits must be [M, A], got {tuple(logits.shape)}")
    M, A = logits.shape
    dev = logits.device
    f = torch.float32
    B = b_logprobs.numel()
    if mb_inds is None and B != M:
        raise ValueError("without mb_inds the batch arrays must have M elements")
    if mb_inds is not None and mb_inds.numel() != M:
        raise ValueError(f"mb_inds has {mb_inds.numel()} elements, logits has M={M} rows")
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    if dvalue is None:
        dvalue = torch.empty(M, dtype=f, device=dev)
    if stats is None:
        stats = torch.empty(len(STAT_NAMES), dtype=f, device=dev)
    if workspace is None:
        workspace = LossWorkspace(M, A, dev)
    call("ocppo_ppo_loss_fwd_bwd", _stream(dev), _check(logits, "logits", f, dev),
         _check(new_value, "new_value", f, dev, M), M, A,
         _opt(mb_inds, "mb_inds", torch.int64, dev, M),
         _check(b_actions, "b_actions", torch.int64, dev, B),
         _check(b_logprobs, "b_logprobs", f, dev, B),
         _check(b_advantages, "b_advantages", f, dev, B), _check(b_returns, "b_returns", f, dev, B),
         _check(b_values, "b_values", f, dev, B),
         _opt(adv_stats, "adv_stats", f, dev, 2) if norm_adv else None,
         float(clip_coef), float(ent_coef), float(vf_coef), int(bool(norm_adv)),
         int(bool(clip_vloss)), _check(dlogits, "dlogits", f, dev, M * A),
         _check(dvalue, "dvalue", f, dev, M), _check(stats, "stats", f, dev, len(STAT_NAMES)),
         workspace.buf.data_ptr(), workspace.nbytes)
    return stats, dlogits, dvalue


# decoder widths ocppo_heads_loss_fwd_bwd is instantiated for (H / 64 columns per lane: 1, 2, 4, 8)
HEADS_LOSS_WIDTHS = (64, 128, 256, 512)


def heads_loss_ok(h, A: int) -> bool:
    H = h.shape[-1]
    return (h.is_cuda and h.dtype == torch.float32 and h.dim() == 2 and h.is_contiguous() and
            H in HEADS_LOSS_WIDTHS and 1 <= A <= 7 and h.data_ptr() % 16 == 0)


class DeferredFinish:
    """The finish of ocppo_heads_loss_rows (the tree over the heads-loss records that writes the
    heads' and decoder-bias gradients and the loss statistics) or of ocppo_relu_bias_wgrad_rows
    (the first layer's dw / db), held as the C-ABI's host record until a later launch on the same
    stream runs it: sum_splits(..., finish=) / sum_splits_db(..., finish=) fold it into a split-K
    combine, run() launches it alone. It must run exactly once (pending: not yet)."""

    def __init__(self, device):
        self.device = device
        self.rec = (ctypes.c_uint64 * 64)()
        self.pending = False  # filled by a rows launch, not yet run
        self.filled = False   # holds a record (a timer replay may run it again: same writes)

    def ptr(self) -> int:
        return ctypes.addressof(self.rec)

    def run(self):
        if self.pending:
            self.pending = False
            call("ocppo_deferred_finish_run", _stream(self.device), self.ptr())


def heads_loss_fwd_bwd(h, wa, ba, wc, bc, mb_actions, mb_logprobs, mb_advantages, mb_returns,
                       mb_values, *, adv_stats, clip_coef, ent_coef, vf_coef, norm_adv: bool,
                       clip_vloss: bool, gp=None, db_h=None, dwa=None, dwc=None, dba=None,
                       dbc=None, stats=None, dlogits=None, dvalue=None, defer=None):
    """The policy heads' forward, the fused PPO loss and the heads' backward with the decoder's
    ReLU mask, from the decoder output h [M, H] (include/ocppo.h ocppo_heads_loss_fwd_bwd).
    mb_* are the minibatch's prepared records [M]. Returns (gp, db_h, dwa, dwc, dba, dbc, stats).
    defer = a DeferredFinish: only the rows kernel runs now (ocppo_heads_loss_rows); db_h, dwa,
    dwc, dba, dbc and stats are written when the caller runs the finish."""
    M, H = h.shape
    A = wa.shape[0]
    dev = h.device
    f = torch.float32
    gp = torch.empty_like(h) if gp is None else gp
    dwa = torch.empty(A, H, dtype=f, device=dev) if dwa is None else dwa
    dwc = torch.empty(1, H, dtype=f, device=dev) if dwc is None else dwc
    dba = torch.empty(A, dtype=f, device=dev) if dba is None else dba
    dbc = torch.empty(1, dtype=f, device=dev) if dbc is None else dbc
    stats = torch.empty(len(STAT_NAMES), dtype=f, device=dev) if stats is None else stats
    ws = _persistent("heads_loss_fwd_bwd", dev, (M, H, A), lambda: torch.zeros(
        int(_lib.LIB.ocppo_heads_loss_workspace_bytes(M, H, A)) // 4, dtype=f, device=dev))
    call("ocppo_heads_loss_rows" if defer is not None else "ocppo_heads_loss_fwd_bwd",
         _stream(dev), _check(h, "h", f, dev, M * H), M, H,
         _check(wa, "wa", f, dev, A * H), _check(ba, "ba", f, dev, A), _check(wc, "wc", f, dev, H),
         _check(bc, "bc", f, dev, 1), A, _check(mb_actions, "mb_actions", torch.int64, dev, M),
         _check(mb_logprobs, "mb_logprobs", f, dev, M),
         _check(mb_advantages, "mb_advantages", f, dev, M),
         _check(mb_returns, "mb_returns", f, dev, M), _check(mb_values, "mb_values", f, dev, M),
         _opt(adv_stats, "adv_stats", f, dev, 2) if norm_adv else None, float(clip_coef),
         float(ent_coef), float(vf_coef), int(bool(norm_adv)), int(bool(clip_vloss)),
         _check(gp, "gp", f, dev, M * H), _opt(db_h, "db_h", f, dev, H),
         _check(dwa, "dwa", f, dev, A * H), _check(dwc, "dwc", f, dev, H),
         _check(dba, "dba", f, dev, A), _check(dbc, "dbc", f, dev, 1),
         _check(stats, "stats", f, dev, len(STAT_NAMES)), _opt(dlogits, "dlogits", f, dev, M * A),
         _opt(dvalue, "dvalue", f, dev, M), ws.data_ptr(), ws.numel() * 4,
         *((defer.ptr(),) if defer is not None else ()))
    if defer is not None:
        defer.pending = defer.filled = True
    return gp, db_h, dwa, dwc, dba, dbc, stats


class _PPOLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, new_value, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                mb_inds, adv_stats, cfg):
        stats, dlogits, dvalue = ppo_loss_fwd_bwd(
            logits.detach().contiguous(), new_value.detach().reshape(-1).contiguous(), b_actions,
            b_logprobs, b_advantages, b_returns, b_values, mb_inds=mb_inds, adv_stats=adv_stats,
            **cfg)
        ctx.save_for_backward(dlogits, dvalue)
        ctx.value_shape = new_value.shape
        ctx.mark_non_differentiable(stats)
        loss = stats[_lib.OCPPO_STAT_LOSS].clone()
        return loss, stats

    @staticmethod
    def backward(ctx, grad_loss, grad_stats):
        dlogits, dvalue = ctx.saved_tensors
        return (dlogits * grad_loss, (dvalue * grad_loss).view(ctx.value_shape), None, None, None,
                None, None, None, None, None)


def ppo_loss(logits, new_value, b_actions, b_logprobs, b_advantages, b_returns, b_values,
             mb_inds=None, adv_stats=None, *, clip_coef, ent_coef, vf_coef, norm_adv=True,
             clip_vloss=True):
    """Differentiable fused PPO loss: returns (loss, stats). Only `loss` carries gradient."""
    cfg = dict(clip_coef=clip_coef, ent_coef=ent_coef, vf_coef=vf_coef, norm_adv=norm_adv,
               clip_vloss=clip_vloss)
    return _PPOLoss.apply(logits, new_value, b_actions, b_logprobs, b_advantages, b_returns,
                          b_values, mb_inds, adv_stats, cfg)


# ---------------------------------------------------------------------------------------------
# Categorical action head (architectures/ppo.py:89-95)
# ---------------------------------------------------------------------------------------------
class TorchExpStream:
    """The reference's sampling stream for the sampling kernels to draw themselves: the Exp(1)
    values torch.empty(N, A).exponential_() would return on `device`'s default generator, one
    [N, A] draw per rollout step (Categorical.sample, architectures/ppo.py:92-94, called at
    ppo_atari_oc.py:505-506). `claim(steps)` (host, before the rollout, outside any graph) takes
    the generator's current (seed, philox offset), advances the generator past `steps` draws as
    `steps` exponential_ calls would, and writes both into the device `state` the captured
    kernels read; `philox(t)` is step t's (state, offset, stride) argument."""

    def __init__(self, numel: int, device):
        self.device = torch.device(device)
        torch.cuda.init()  # default_generators is empty until the runtime is initialised
        self.gen = torch.cuda.default_generators[self.device.index
                                                 if self.device.index is not None else 0]
        self.stride, self.increment = torch_exponential_geometry(numel, self.device)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._seed = None

    def claim(self, steps: int):
        base = self.gen.get_offset()
        self.gen.set_offset(base + steps * self.increment)
        seed = self.gen.initial_seed()
        if seed != self._seed:
            self.state[0].fill_(seed if seed < 1 << 63 else seed - (1 << 64))
            self._seed = seed
        self.state[1].fill_(base)  # a fill launch with the value as argument: no host sync

    def philox(self, t: int):
        return self.state, t * self.increment, self.stride

    def fill(self, noise):
        """noise [T, ...] = the T claimed draws (one launch; graph-capturable)."""
        return philox_exponential_steps(noise, self.state, 0, self.increment, self.stride)


def torch_exponential_geometry(numel: int, device) -> tuple[int, int]:
    """(grid stride, philox-offset increment) of torch's exponential_ over `numel` elements on
    `device` (ocppo_torch_exponential_geometry)."""
    props = torch.cuda.get_device_properties(device)
    stride, inc = ctypes.c_int64(), ctypes.c_int64()
    call("ocppo_torch_exponential_geometry", numel, props.multi_processor_count,
         props.max_threads_per_multi_processor, ctypes.byref(stride), ctypes.byref(inc))
    return stride.value, inc.value


def philox_exponential(out, state, offset: int, stride: int):
    """out[:] = torch's exponential_ draws at generator state[0..1] + (0, offset)."""
    dev = out.device
    call("ocppo_philox_exponential", _stream(dev), _check(out, "out", torch.float32, dev),
         out.numel(), _check(state, "philox_state", torch.int64, dev, 2), int(offset), int(stride))
    return out


def philox_exponential_steps(out, state, offset: int, increment: int, stride: int):
    """out[t] = torch's exponential_ draw t of shape out[0] at generator state[0..1] + (0, offset +
    t * increment): a rollout's per-step draws in one launch (out [steps, ...])."""
    dev = out.device
    steps = out.shape[0]
    call("ocppo_philox_exponential_steps", _stream(dev), _check(out, "out", torch.float32, dev),
         out[0].numel(), steps, _check(state, "philox_state", torch.int64, dev, 2), int(offset),
         int(increment), int(stride))
    return out


def _noise_args(noise, philox, n, dev):
    """(noise pointer, philox state pointer, offset, stride) of a sampling entry: noise read, or
    philox = (state, offset, stride) drawn in the kernel (noise then optional, written)."""
    f = torch.float32
    if philox is None:
        return (_check(noise, "noise", f, dev, n), None, 0, 0)
    state, off, stride = philox
    return (_opt(noise, "noise", f, dev, n), _check(state, "philox_state", torch.int64, dev, 2),
            int(off), int(stride))


def categorical_sample(logits, noise, action_out=None, logprob_out=None, entropy_out=None,
                       value_in=None, value_out=None, philox=None):
    """argmax(softmax(logits) / noise) with log_prob and entropy; noise ~ Exp(1) [N, A] (or drawn
    in the kernel: philox = TorchExpStream.philox(t), noise then receives the draws if given)."""
    N, A = logits.shape
    dev = logits.device
    f = torch.float32
    if action_out is None:
        action_out = torch.empty(N, dtype=torch.int64, device=dev)
    if logprob_out is None:
        logprob_out = torch.empty(N, dtype=f, device=dev)
    if (value_in is None) != (value_out is None):
        raise ValueError("value_in and value_out go together")
    call("ocppo_categorical_sample", _stream(dev), _check(logits, "logits", f, dev),
         *_noise_args(noise, philox, N * A, dev), N, A,
         _check(action_out, "action_out", torch.int64, dev, N),
         _check(logprob_out, "logprob_out", f, dev, N), _opt(entropy_out, "entropy_out", f, dev, N),
         _opt(value_in, "value_in", f, dev, N), _opt(value_out, "value_out", f, dev, N))
    return action_out, logprob_out, entropy_out


def policy_head_sample(hidden, w_actor, b_actor, w_critic, b_critic, noise, action_out=None,
                       logprob_out=None, value_out=None, entropy_out=None, logits_out=None,
                       philox=None):
    """Fused actor/critic heads + Categorical sample for a rollout step (no autograd)."""
    N, H = hidden.shape
    A = w_actor.shape[0]
    dev = hidden.device
    f = torch.float32
    if tuple(w_actor.shape) != (A, H) or w_critic.numel() != H or b_actor.numel() != A:
        raise ValueError("head weights do not match hidden")
    if action_out is None:
        action_out = torch.empty(N, dtype=torch.int64, device=dev)
    if logprob_out is None:
        logprob_out = torch.empty(N, dtype=f, device=dev)
    if value_out is None:
        value_out = torch.empty(N, dtype=f, device=dev)
    call("ocppo_policy_head_sample", _stream(dev), _check(hidden, "hidden", f, dev), N, H,
         _check(w_actor, "w_actor", f, dev), _check(b_actor, "b_actor", f, dev, A),
         _check(w_critic, "w_critic", f, dev, H), _check(b_critic, "b_critic", f, dev, 1),
         *_noise_args(noise, philox, N * A, dev), A,
         _check(action_out, "action_out", torch.int64, dev, N),
         _check(logprob_out, "logprob_out", f, dev, N), _opt(entropy_out, "entropy_out", f, dev, N),
         _check(value_out, "value_out", f, dev, N), _opt(logits_out, "logits_out", f, dev, N * A))
    return action_out, logprob_out, value_out


def policy_head_env_ok(hidden, w_actor, w_critic, env) -> bool:
    """policy_head_env_step applies: the E = 1 head form and an object-frame synthetic env."""
    N, H = hidden.shape
    A = w_actor.shape[0]
    fr = getattr(env, "frame", None)
    return (getattr(env, "synthetic", False) and fr is not None and fr.dtype == torch.float32
            and fr.is_contiguous() and 1 <= fr.shape[1] <= 4096 and fr.shape[0] == N
            and 1 <= N <= (3072 if H <= 512 else 2048) and H % 256 == 0 and 256 <= H <= 1024
            and 1 <= A <= 7 and hidden.is_contiguous() and w_actor.is_contiguous()
            and w_critic.is_contiguous()
            and (hidden.data_ptr() | w_actor.data_ptr() | w_critic.data_ptr()) % 16 == 0)


def policy_head_env_step(hidden, w_actor, b_actor, w_critic, b_critic, noise, action_out,
                         logprob_out, value_out, env, step_offset: int, philox=None):
    """policy_head_sample + env.step(action_out, step_offset) in one launch
    (ocppo_policy_head_env_step; env a SyntheticAtariEnv with object frames)."""
    N, H = hidden.shape
    A = w_actor.shape[0]
    dev = hidden.device
    f = torch.float32
    if tuple(w_actor.shape) != (A, H) or w_critic.numel() != H or b_actor.numel() != A:
        raise ValueError("head weights do not match hidden")
    D = env.frame.shape[1]
    call("ocppo_policy_head_env_step", _stream(dev), _check(hidden, "hidden", f, dev), N, H,
         _check(w_actor, "w_actor", f, dev), _check(b_actor, "b_actor", f, dev, A),
         _check(w_critic, "w_critic", f, dev, H), _check(b_critic, "b_critic", f, dev, 1),
         *_noise_args(noise, philox, N * A, dev), A,
         _check(action_out, "action_out", torch.int64, dev, N),
         _check(logprob_out, "logprob_out", f, dev, N), _check(value_out, "value_out", f, dev, N),
         env.seed & 0xFFFFFFFFFFFFFFFF, _check(env.step_base, "step_base", torch.int64, dev, 1),
         int(step_offset), D, _check(env.frame, "frame", f, dev, N * D),
         _check(env.reward, "reward", f, dev, N), _check(env.done, "done", f, dev, N),
         _opt(env.ep_state, "ep_state", f, dev, N * 5))
    return action_out, logprob_out, value_out


class _CategoricalLogProbEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, actions):
        N, A = logits.shape
        dev = logits.device
        lp = torch.empty(N, dtype=torch.float32, device=dev)
        ent = torch.empty(N, dtype=torch.float32, device=dev)
        lg = logits.detach().contiguous()
        act = actions.detach().reshape(-1).long().contiguous()
        call("ocppo_categorical_logprob_entropy", _stream(dev),
             _check(lg, "logits", torch.float32, dev), _check(act, "actions", torch.int64, dev, N),
             N, A, lp.data_ptr(), ent.data_ptr())
        ctx.save_for_backward(lg, act)
        return lp, ent

    @staticmethod
    def backward(ctx, g_lp, g_ent):
        lg, act = ctx.saved_tensors
        N, A = lg.shape
        dev = lg.device
        dl = torch.empty_like(lg)
        g_lp = None if g_lp is None else g_lp.contiguous()
        g_ent = None if g_ent is None else g_ent.contiguous()
        call("ocppo_categorical_logprob_entropy_bwd", _stream(dev), lg.data_ptr(), act.data_ptr(),
             _opt(g_lp, "grad_logprob", torch.float32, dev, N),
             _opt(g_ent, "grad_entropy", torch.float32, dev, N), N, A, dl.data_ptr())
        return dl, None


def categorical_logprob_entropy(logits, actions):
    """(log_prob(actions), entropy()) of Categorical(logits=logits), differentiable in logits."""
    return _CategoricalLogProbEntropy.apply(logits, actions)


# ---------------------------------------------------------------------------------------------
# rollout store / reset (ppo_atari_oc.py:502-503, 512-514), minibatch gather (:566-567)
# ---------------------------------------------------------------------------------------------
def _reset_prev(reset_prev, frame, N: int, W: int, D: int, dev):
    if reset_prev is None:
        return None
    if reset_prev.dtype != frame.dtype:
        raise ValueError(f"reset_prev dtype {reset_prev.dtype} != frame dtype {frame.dtype}")
    return _check(reset_prev, "reset_prev", None, dev, N * (W - 1) * D)


def rollout_store(frame, reward, done, prev_obs, obs_out, net_obs=None, reward_out=None,
                  done_out=None, scale255: bool = False, reset_prev=None):
    """obs_out = stack(prev_obs[:, 1:], frame) (reset-filled where done), plus reward/done rows.

    frame [N, D] f32|u8; prev_obs/obs_out [N, W, D] f32|bf16|u8; net_obs [N, W, D] f32, or a
    channels_last [N, W, H, X] f32 tensor (written in NHWC order). scale255: net_obs holds
    value / 255 exactly as the NatureCNN's NormalizeImg computes it on the GPU. reset_prev
    [N, W-1, D] (frame dtype): the older frames of the env's own reset observation for done rows
    (None: FrameStack's fill with the newest frame).
    """
    N, D = frame.shape[0], frame[0].numel()
    W = obs_out.shape[1]
    dev = frame.device
    if tuple(obs_out.shape[:2]) != (N, W) or obs_out[0, 0].numel() != D:
        raise ValueError(f"obs_out {tuple(obs_out.shape)} does not match frame {tuple(frame.shape)}")
    if prev_obs.shape != obs_out.shape or prev_obs.dtype != obs_out.dtype:
        raise ValueError("prev_obs and obs_out must have the same shape and dtype")
    if frame.dtype not in (torch.float32, torch.uint8) or obs_out.dtype not in _DTYPE_CODE:
        raise ValueError(f"unsupported dtypes frame={frame.dtype} obs={obs_out.dtype}")
    f = torch.float32
    net, layout = _net_obs(net_obs, N, W, D, dev)
    call("ocppo_rollout_store", _stream(dev), _check(frame, "frame", None, dev),
         _DTYPE_CODE[frame.dtype], _check(reward, "reward", f, dev, N),
         _check(done, "done", f, dev, N), N, W, D, _check(prev_obs, "prev_obs", None, dev),
         _check(obs_out, "obs_out", None, dev), _DTYPE_CODE[obs_out.dtype], net,
         _opt(reward_out, "reward_out", f, dev, N), _opt(done_out, "done_out", f, dev, N),
         layout | (OCPPO_NET_SCALE_255 if scale255 else 0),
         _reset_prev(reset_prev, frame, N, W, D, dev))


def rollout_store_vecnorm(frame, reward, done, prev_obs, obs_out, net_obs, done_out, ret_state,
                          rms_state, reward_out, gamma=0.99, epsilon=1e-8, clip_reward=10.0,
                          scale255: bool = False, reset_prev=None):
    """rollout_store + vecnorm_reward in one launch (reward_out gets the normalised reward)."""
    N, D = frame.shape[0], frame[0].numel()
    W = obs_out.shape[1]
    dev = frame.device
    if prev_obs.shape != obs_out.shape or prev_obs.dtype != obs_out.dtype:
        raise ValueError("prev_obs and obs_out must have the same shape and dtype")
    if tuple(obs_out.shape[:2]) != (N, W) or obs_out[0, 0].numel() != D:
        raise ValueError(f"obs_out {tuple(obs_out.shape)} does not match frame {tuple(frame.shape)}")
    f = torch.float32
    net, layout = _net_obs(net_obs, N, W, D, dev)
    call("ocppo_rollout_store_vecnorm", _stream(dev), _check(frame, "frame", None, dev),
         _DTYPE_CODE[frame.dtype], _check(reward, "reward", f, dev, N),
         _check(done, "done", f, dev, N), N, W, D, _check(prev_obs, "prev_obs", None, dev),
         _check(obs_out, "obs_out", None, dev), _DTYPE_CODE[obs_out.dtype], net,
         _opt(done_out, "done_out", f, dev, N),
         float(gamma), float(epsilon), float(clip_reward),
         _check(ret_state, "ret_state", torch.float64, dev, N),
         _check(rms_state, "rms_state", torch.float64, dev, 3),
         _check(reward_out, "reward_out", f, dev, N),
         layout | (OCPPO_NET_SCALE_255 if scale255 else 0),
         _reset_prev(reset_prev, frame, N, W, D, dev))


def obs_reset(frame, obs_out, net_obs=None, scale255: bool = False):
    N, D = frame.shape[0], frame[0].numel()
    W = obs_out.shape[1]
    dev = frame.device
    if obs_out.numel() != N * W * D:
        raise ValueError("obs_out does not match frame")
    net, layout = _net_obs(net_obs, N, W, D, dev)
    call("ocppo_obs_reset", _stream(dev), _check(frame, "frame", None, dev),
         _DTYPE_CODE[frame.dtype], N, W, D, _check(obs_out, "obs_out", None, dev),
         _DTYPE_CODE[obs_out.dtype], net, layout | (OCPPO_NET_SCALE_255 if scale255 else 0))


def linear_act(x, weight, bias=None, relu: bool = False, out=None, ring=None):
    """y = act(x @ weight.T + bias) on the f32 matrix cores, for rollout-sized batches (no
    autograd). x [M, K] f32 with unit column stride (row stride may exceed K, e.g. a frame slice
    of the stacked obs); weight [N, K] contiguous (nn.Linear.weight); bias [N] or None.
    ring = (seg, rot): x's rows are K / seg segments stored rotated, logical segment s at
    physical (s + rot) mod (K / seg) (the frame-encoding ring, ocppo_linear_act_ring)."""
    if x.dim() != 2 or weight.dim() != 2:
        raise ValueError(f"x must be [M, K] and weight [N, K], got {tuple(x.shape)}, "
                         f"{tuple(weight.shape)}")
    M, K = x.shape
    N = weight.shape[0]
    dev = x.device
    if weight.shape[1] != K:
        raise ValueError(f"weight is {tuple(weight.shape)}, x has K={K}")
    if x.dtype != torch.float32 or (M > 1 and x.stride(1) != 1) or x.device.type != "cuda":
        raise ValueError("x must be an f32 GPU tensor with unit column stride")
    ldx = x.stride(0) if M > 1 else K
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (M, N) or (M > 1 and out.stride(1) != 1) or out.dtype != torch.float32:
        raise ValueError("out must be an f32 [M, N] tensor with unit column stride")
    ldy = out.stride(0) if M > 1 else N
    if ring is not None:
        seg, rot = (int(v) for v in ring)
        call("ocppo_linear_act_ring", _stream(dev), x.data_ptr(), ldx,
             _check(weight, "weight", torch.float32, dev), _opt(bias, "bias", torch.float32, dev, N),
             out.data_ptr(), ldy, M, N, K, seg, rot, 1 if relu else 0)
        return out
    call("ocppo_linear_act", _stream(dev), x.data_ptr(), ldx,
         _check(weight, "weight", torch.float32, dev), _opt(bias, "bias", torch.float32, dev, N),
         out.data_ptr(), ldy, M, N, K, 1 if relu else 0)
    return out


def conv2d_act(x, weight, bias=None, stride: int = 1, relu: bool = True, out=None):
    """act(conv2d(x, weight, bias, stride)) on the f32 matrix cores (ocppo_conv2d_act) for
    channels_last tensors: x [B, Cin, H, W] and weight [Cout, Cin, KH, KW] both in
    torch.channels_last memory format; no padding / dilation / groups. Returns [B, Cout, OH, OW]
    in channels_last (no autograd: the rollout forward)."""
    B, Cin, H, W = x.shape
    Cout, Cw, KH, KW = weight.shape
    dev = x.device
    f = torch.float32
    cl = torch.channels_last
    if Cw != Cin or x.dtype != f or weight.dtype != f or x.device.type != "cuda":
        raise ValueError("conv2d_act: f32 GPU x [B, Cin, H, W] and weight [Cout, Cin, KH, KW]")
    if not (x.is_contiguous(memory_format=cl) and weight.is_contiguous(memory_format=cl)):
        raise ValueError("conv2d_act: x and weight must be channels_last")
    OH, OW = (H - KH) // stride + 1, (W - KW) // stride + 1
    if out is None:
        out = torch.empty((B, Cout, OH, OW), dtype=f, device=dev, memory_format=cl)
    if tuple(out.shape) != (B, Cout, OH, OW) or not out.is_contiguous(memory_format=cl):
        raise ValueError("conv2d_act: out must be a channels_last [B, Cout, OH, OW] tensor")
    call("ocppo_conv2d_act", _stream(dev), x.data_ptr(), B, H, W, Cin, weight.data_ptr(),
         _opt(bias, "bias", f, dev, Cout), Cout, KH, KW, stride, out.data_ptr(), int(bool(relu)))
    return out


# ---- NHWC convolutions as implicit GEMMs on the x6 products (ocppo_conv_x6) ---------------------
# The NatureCNN trunk (architectures/ppo.py:20-31) without MIOpen: forward, weight gradient and
# data gradient, deterministic (split-K partials summed in split order), f32-level products.
_CONV_TILES = {0: (128, 32), 1: (32, 128), 2: (128, 64), 3: (64, 64), 4: (64, 128), 5: (128, 128),
               6: (32, 64)}


CONV_FWD_MIN_UNITS = 512


def _conv_fwd_tile(M: int, N: int) -> int | None:
    """The largest tile giving >= CONV_FWD_MIN_UNITS workgroups (two per CU), else the one giving
    the most."""
    best, units = None, 0
    for t in ((0,) if N == 32 else (2, 3, 6) if N == 64 else (5, 2, 3, 6)):
        bm, bn = _CONV_TILES[t]
        if M % bm == 0 and N % bn == 0:
            u = (M // bm) * (N // bn)
            if u >= CONV_FWD_MIN_UNITS:
                return t
            if u > units:
                best, units = t, u
    return best


def _conv_wgrad_tile(M: int, N: int) -> int | None:
    for t in ((1,) if M == 32 else (4, 3) if M == 64 else (5, 4, 3)):
        bm, bn = _CONV_TILES[t]
        if M % bm == 0 and N % bn == 0:
            return t
    return None


def conv_x6_ok(x, weight, stride: int, wgrad: bool = False, dgrad: bool = False) -> bool:
    """Shapes ocppo_conv_x6 takes: channels_last f32 x [B, C, H, W] and weight [Cout, C, KH, KW]
    (square stride, no padding), C % 4 == 0, kernel rows of KW C % 32 == 0 taps, row counts the
    tiles divide; wgrad / dgrad: also the weight gradient / the data gradient's stride classes."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and weight.dim() == 4 and weight.dtype == torch.float32):
        return False
    cl = torch.channels_last
    if not (x.is_contiguous(memory_format=cl) and weight.is_contiguous(memory_format=cl)):
        return False
    B, C, H, W = x.shape
    Cout, Cw, KH, KW = weight.shape
    s = int(stride)
    if Cw != C or C % 4 or (KW * C) % 32 or H < KH or W < KW or (H - KH) % s or (W - KW) % s:
        return False
    OH, OW = (H - KH) // s + 1, (W - KW) // s + 1
    rows = B * OH * OW
    if rows >= 1 << 24 or _conv_fwd_tile(rows, Cout) is None:
        return False
    if wgrad and (OH * OW > 1024 or rows % 32 or _conv_wgrad_tile(Cout, KH * KW * C) is None):
        return False
    if dgrad:
        if KH % s or KW % s or H % s or W % s or Cout % 4 or ((KW // s) * Cout) % 32:
            return False
        qrows = B * (H // s) * (W // s)
        return qrows < 1 << 24 and _conv_fwd_tile(qrows, s * s * C) is not None
    return True


# weight gradients: K splits for about this many workgroups (each split's partial [Cout, N] summed
# in split order by the same launch's sum_parts), per tile; measured at config 3's minibatch of
# 8192 (profiles/r05/ab_conv_wgrad_units.txt): 32 x 128 (the first layer) and 64 x 128 best at
# 1024, 64 x 64 at 4096. None: the per-tile table; an int: one target for every tile
CONV_WGRAD_UNITS = None
_WGRAD_UNITS = {1: 1024, 4: 1024, 3: 4096}


def _wgrad_units(tile: int) -> int:
    return CONV_WGRAD_UNITS if CONV_WGRAD_UNITS else _WGRAD_UNITS.get(tile, 2048)


def _geom(*v):
    return (ctypes.c_int64 * len(v))(*[int(t) for t in v])


# Bounds-check builds of the library (`python tools/build_variant.py OUT.so -DOCPPO_X6_BOUNDS`,
# loaded with OCPPO_LIB=OUT.so; never the product): before every convolution launch the library
# is handed the extents of the sources its gathers read, from the pointers it is passed, and a
# device record of the first out-of-range index (tests/test_conv_bounds_gpu.py reads it).
# The probe is no part of the C-ABI (the header does not declare it), hence the lookup by name.
_X6_PROBE = getattr(_lib.LIB, "ocppo_x6_probe_set_bounds", None)
X6_BOUNDS = _X6_PROBE is not None
if X6_BOUNDS:
    _X6_PROBE.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
BOUND_KINDS = {1: "f32 source offset", 2: "image index", 3: "u8 stack row", 4: "u8 byte offset"}


def _tail(t) -> int:
    """Elements of t's storage from t's first element on."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def bounds_record(dev) -> torch.Tensor:
    """The bounds-check build's violation record on `dev` (int32 [count, first kind, first index
    lo, hi, its limit lo, hi, 0, 0])."""
    return _persistent("bounds_record", dev, (),
                       lambda: torch.zeros(8, dtype=torch.int32, device=dev))


def __getattr__(name):
    if name == "_BOUNDS_REC":  # every device's record, by device (the suite's fixture reads it)
        return {str(k[1]): v for k, v in _PERSISTENT.items() if k[0] == "bounds_record"}
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _bounds(dev, x=None, u8=None):
    if X6_BOUNDS:
        _X6_PROBE(bounds_record(dev).data_ptr(), _tail(x) if x is not None else 0,
                  _tail(u8) if u8 is not None else 0, u8.shape[0] if u8 is not None else 0)


def _conv_rows_form(M: int, Cout: int) -> bool:
    """conv_x6 takes the few-rows form (ocppo_conv_x6 tile 7) for this product."""
    return CONV_FWD_ROWS and M <= CONV_FWD_ROWS_MAX and Cout in (32, 64) and M % 32 == 0


def _conv_planes_ptr(w_planes, N: int, K: int, dev):
    if w_planes is None:
        return None
    if w_planes.dtype != torch.bfloat16 or tuple(w_planes.shape) != (3, N, K) or \
            not w_planes.is_contiguous():
        raise ValueError(f"conv_x6: w_planes must be contiguous bf16 [3, {N}, {K}]")
    return _check(w_planes, "w_planes", torch.bfloat16, dev)


def conv_x6(x, weight, bias=None, stride: int = 1, relu: bool = True, out=None, w_planes=None,
            mbits=None):
    """act(conv2d(x, weight) + bias) (architectures/ppo.py:20-31's Conv2d + ReLU) on ocppo_conv_x6:
    channels_last f32 x [B, C, H, W], weight [Cout, C, KH, KW] -> channels_last [B, Cout, OH, OW]
    (no autograd; agents._ConvX6 is the autograd form). w_planes: the weight's [Cout, KH KW C]
    matrix pre-split into bf16 [3, Cout, KH KW C] (ocppo_split_planes: the same pieces as the
    in-kernel split, so the same bits). mbits: an int32 [B OH OW Cout / 32] tensor the tile loop's
    epilogue fills with the output's ReLU mask, row-major (relu_bias_grad's bits= form); the
    few-rows form (no autograd) takes none."""
    if not conv_x6_ok(x, weight, stride):
        raise ValueError(f"conv_x6: unsupported shapes x {tuple(x.shape)}, weight "
                         f"{tuple(weight.shape)}, stride {stride} (conv_x6_ok)")
    B, C, H, W = x.shape
    Cout, _, KH, KW = weight.shape
    s = int(stride)
    OH, OW = (H - KH) // s + 1, (W - KW) // s + 1
    dev, f = x.device, torch.float32
    K = KH * KW * C
    M = B * OH * OW
    wm = weight.permute(0, 2, 3, 1).reshape(Cout, K)  # a view: [Cout, KH, KW, C] in memory
    if out is None:
        out = torch.empty((B, Cout, OH, OW), dtype=f, device=dev, memory_format=torch.channels_last)
    if tuple(out.shape) != (B, Cout, OH, OW) or not out.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("conv_x6: out must be a channels_last [B, Cout, OH, OW] tensor")
    geom = _geom(OH, OW, H * W * C, s * W * C, s * C, W * C, KW * C)
    if _conv_rows_form(M, Cout):
        # few rows (the rollout's batch): K steps split over the waves of a workgroup
        if mbits is not None:
            raise ValueError("conv_x6: the few-rows form writes no ReLU bitmask")
        _bounds(dev, x)
        call("ocppo_conv_x6", _stream(dev), 0, x.data_ptr(), geom, wm.data_ptr(), K,
             out.data_ptr(), Cout, M, Cout, K, 1, _opt(bias, "bias", f, dev, Cout),
             int(bool(relu)), None, 7, None, None, None, None,
             _conv_planes_ptr(w_planes, Cout, K, dev), None)
        return out
    tile = _conv_fwd_tile(M, Cout)
    bm, bn = _CONV_TILES[tile]
    S = _conv_fwd_splits((M // bm) * (Cout // bn), K // 32)
    _bounds(dev, x)
    wpp = _conv_planes_ptr(w_planes, Cout, K, dev)
    if mbits is not None and (S != 1 or not relu or Cout % 32):
        raise ValueError("conv_x6: mbits needs one product with relu, 32 | Cout")
    if S == 1:
        call("ocppo_conv_x6", _stream(dev), 0, x.data_ptr(), geom, wm.data_ptr(), K,
             out.data_ptr(), Cout, M, Cout, K, 1, _opt(bias, "bias", f, dev, Cout),
             int(bool(relu)), None, tile, None, None, None, None, wpp,
             _opt(mbits, "mbits", torch.int32, dev, M * Cout // 32))
        return out
    # few rows (the rollout's batch): K-split partials, then bias + ReLU on their ordered sum
    part = _persistent("conv_x6", dev, (S, M, Cout),
                       lambda: torch.empty((S, M, Cout), dtype=f, device=dev))
    call("ocppo_conv_x6", _stream(dev), 0, x.data_ptr(), geom, wm.data_ptr(), K, part.data_ptr(),
         Cout, M, Cout, K, S, None, 0, None, tile, None, None, None, None, wpp, None)
    call("ocppo_sum_splits_act", _stream(dev), part.data_ptr(), S, M, Cout,
         _opt(bias, "bias", f, dev, Cout), int(bool(relu)), out.data_ptr())
    return out


# Forward products of at most CONV_FWD_ROWS_MAX rows (the rollout's batch: 20736 / 12544 rows for
# NatureCNN's second / third layer at 256 envs) on ocppo_conv_x6 tile 7: a 32-row tile per
# workgroup, its K steps split over 8 waves and summed through LDS in wave order, instead of the
# tile loop's chain of 16-18 dependent K steps on 2 waves
CONV_FWD_ROWS = True
CONV_FWD_ROWS_MAX = 65536


# K splits for a forward product of few workgroups (< 512; the rollout's image batch): measured
# no faster at 256 envs (conv + ordered sum 23.8 / 24.6 / 25.4 us vs 23.5 / 24.5 / 25.1 us in one
# launch), so off by default
CONV_FWD_SPLITS = False


def _conv_fwd_splits(units: int, steps: int) -> int:
    if not CONV_FWD_SPLITS or units >= 512:
        return 1
    S = 1
    for c in (2, 4, 8):
        if steps // c < 3:
            break
        S = c
        if units * c >= 1024:
            break
    return S


def conv_x6_wgrad(gp, x, kernel: tuple, stride: int, out=None):
    """dW of a convolution (channels_last weight layout [Cout, KH, KW, C] as a [Cout, KH KW C]
    matrix): sum over the output pixels r of gp[r, co] x(r, (ky, kx, c)); gp [B OH OW, Cout] the
    output gradient's NHWC rows, x the channels_last input. Split-K partials summed in order."""
    B, C, H, W = x.shape
    KH, KW = kernel
    s = int(stride)
    OH, OW = (H - KH) // s + 1, (W - KW) // s + 1
    rows, Cout = gp.shape
    dev, f = x.device, torch.float32
    if rows != B * OH * OW or not x.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("conv_x6_wgrad: gp must be [B OH OW, Cout], x channels_last")
    N = KH * KW * C
    tile = _conv_wgrad_tile(Cout, N)
    if tile is None or rows % 32:
        raise ValueError(f"conv_x6_wgrad: no tile for [{Cout} x {N}] over {rows} rows")
    bm, bn = _CONV_TILES[tile]
    tiles = (Cout // bm) * (N // bn)
    S = max(1, min(rows // 32 // 32, _wgrad_units(tile) // tiles))
    part = _persistent("conv_x6_wgrad", dev, (S, Cout, N),
                       lambda: torch.empty((S, Cout, N), dtype=f, device=dev))
    if out is None:
        out = torch.empty((Cout, N), dtype=f, device=dev)
    if out.numel() != Cout * N or not out.is_contiguous(memory_format=torch.channels_last
                                                        if out.dim() == 4 else torch.contiguous_format):
        raise ValueError("conv_x6_wgrad: out must hold [Cout, KH KW C] contiguously")
    _bounds(dev, x)
    call("ocppo_conv_x6", _stream(dev), 1, x.data_ptr(),
         _geom(OH, OW, H * W * C, s * W * C, s * C, W * C, KW * C),
         _check(gp, "gp", f, dev), Cout, part.data_ptr(), N, Cout, N, rows, S, None, 0, None, tile,
         out.data_ptr(), None, None, None, None, None)
    return out


def conv_x6_dgrad_fuses_relu(M: int, C: int, stride: int) -> bool:
    """conv_x6_dgrad can take the layer below's ReLU backward (the bounded loader's tiles)."""
    return not CONV_DGRAD_PAD_COPY and _conv_fwd_tile(M, stride * stride * C) in (2, 3, 5, 6)


def conv_x6_dgrad(gp, weight, stride: int, in_hw: tuple, out=None, relu_out=None, db=None):
    """dX of a convolution: gp channels_last [B, Cout, OH, OW] (the output gradient), weight
    [Cout, C, KH, KW] -> channels_last [B, C, H, W]. Per stride class (py, px) a forward-form
    product over gp zero-padded by KH / s - 1 with that class's taps flipped; each input pixel
    gets its <= (KH / s)^2 taps in one fixed order (deterministic). relu_out: the layer below's
    ReLU output (channels_last [B, C, H, W]): its ReLU backward in the epilogue (dX masked where
    relu_out <= 0) and its bias gradient (the masked dX's per-channel sums, row tiles and classes
    added in order in f64) into db [C]."""
    B, Cout, OH, OW = gp.shape
    _, C, KH, KW = weight.shape
    H, W = in_hw
    s = int(stride)
    T, TW = KH // s, KW // s
    dev, f = gp.device, torch.float32
    g = gp.permute(0, 2, 3, 1)  # NHWC view
    if not g.is_contiguous():
        g = g.contiguous()
    Hp, Wp = OH + 2 * (T - 1), OW + 2 * (TW - 1)
    QH, QW = H // s, W // s
    M, K = B * QH * QW, T * TW * Cout
    N = s * s * C  # every stride class's C channels: the classes read the same gradient rows
    tile = _conv_fwd_tile(M, N)
    if CONV_DGRAD_TILE and M % _CONV_TILES[CONV_DGRAD_TILE][0] == 0 and \
            N % _CONV_TILES[CONV_DGRAD_TILE][1] == 0:
        tile = CONV_DGRAD_TILE
    if out is None:
        out = torch.empty((B, C, H, W), dtype=f, device=dev, memory_format=torch.channels_last)
    if tuple(out.shape) != (B, C, H, W) or not out.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("conv_x6_dgrad: out must be a channels_last [B, C, H, W] tensor")
    # class (py, px)'s taps ky = py + s t, flipped (t' = T - 1 - t), as [C, T, TW, Cout] rows;
    # the classes stacked class-major: B = [s s C, K] -- one gather through a cached index into
    # the weight's memory (its [Cout, KH, KW, C] order when channels_last) instead of s^2 flips,
    # a stack and a layout copy per call
    wc, wcp = _dgrad_weight(weight, s, planes=CONV_DGRAD_PLANES and
                            (tile != 5 or CONV_DGRAD_PLANES_128))
    wpp = None if wcp is None else wcp.data_ptr()
    og = None if s == 1 else _geom(H * W * C, s * W * C, s * C, 0, C, s, W * C, C)
    if CONV_DGRAD_PAD_COPY or tile not in (2, 3, 5, 6):
        gpad = torch.nn.functional.pad(g, (0, 0, TW - 1, TW - 1, T - 1, T - 1))
        if relu_out is not None:
            raise ValueError("conv_x6_dgrad: the ReLU epilogue needs the bounded loader")
        _bounds(dev, gpad)
        call("ocppo_conv_x6", _stream(dev), 0, gpad.data_ptr(),
             _geom(QH, QW, Hp * Wp * Cout, Wp * Cout, Cout, Wp * Cout, TW * Cout), wc.data_ptr(),
             K, out.data_ptr(), C, M, N, K, 1, None, 0, og, tile, None, None, None, None, wpp, None)
        return out
    # the padding as bounds in the loader: taps outside the gradient read as zeros
    mask = dbp = None
    if relu_out is not None:
        if tuple(relu_out.shape) != (B, C, H, W) or not relu_out.is_contiguous(
                memory_format=torch.channels_last) or db is None:
            raise ValueError("conv_x6_dgrad: relu_out must be channels_last [B, C, H, W], with db")
        mask = relu_out
        dbp = torch.empty((M // _CONV_TILES[tile][0], N), dtype=f, device=dev)
    _bounds(dev, g)
    call("ocppo_conv_x6", _stream(dev), 0, g.data_ptr(),
         _geom(QH, QW, 0, 0, 0, 0, TW * Cout), wc.data_ptr(), K, out.data_ptr(), C, M, N, K, 1,
         None, 0, og, tile, None, _geom(T - 1, TW - 1, OH, OW, Cout),
         None if mask is None else mask.data_ptr(), None if dbp is None else dbp.data_ptr(), wpp, None)
    if dbp is not None:
        # row tiles, then stride classes, in order (f64, one rounding)
        db.copy_(dbp.view(-1, s * s, C).double().sum(0).sum(0))
    return out


# the data gradients' B operand (the stride classes' flipped weights) pre-split into bf16 planes
# once per call (ocppo_split_planes) instead of in every workgroup of the product
CONV_DGRAD_PLANES = True
# ... also on the 128 x 128 tile (the conv2 data gradient's 4 x 32 class columns), whose pre-split
# instance spills (experiments: A/B)
CONV_DGRAD_PLANES_128 = True


def _dgrad_weight(weight, s: int, planes: bool = False):
    """(wc, its bf16 planes or None): conv_x6_dgrad's B operand [s s C, T TW Cout], row (py, px,
    c), column (t, tw, co) = weight[co, c, py + s (T - 1 - t), px + s (TW - 1 - tw)], gathered in
    one launch into a buffer the weight owns (weight._ocppo_dgrad[s]: its own, freed with it; and
    split into planes by one more launch)."""
    Cout, C, KH, KW = weight.shape
    mem = weight.permute(0, 2, 3, 1)  # a view of the memory when channels_last
    dev = weight.device

    def make_idx():
        ar = torch.arange(Cout * KH * KW * C).view(Cout, KH, KW, C).permute(0, 3, 1, 2)
        idx = torch.stack([ar[:, :, py::s, px::s].flip(2, 3).permute(1, 2, 3, 0)
                           for py in range(s) for px in range(s)])
        return idx.reshape(s * s * C, -1).to(dev)

    idx = _persistent("_dgrad_weight", dev, (Cout, C, KH, KW, s), make_idx)
    own = weight.__dict__.setdefault("_ocppo_dgrad", {})
    ent = own.get(s)
    if ent is None:
        ent = own[s] = [torch.empty(idx.shape, dtype=torch.float32, device=dev), None]
    buf = ent[0]
    with torch.no_grad():  # (the kernel timer replays this outside autograd's backward)
        torch.index_select(mem.reshape(-1), 0, idx.view(-1), out=buf.view(-1))
    if not planes or buf.shape[1] % 8:
        return buf, None
    if ent[1] is None:
        ent[1] = WeightPlanes(fwd=(buf,))
    ent[1].refresh()
    return buf, buf._ocppo_planes["fwd"]


# an explicit tile for the data gradients (0: _conv_fwd_tile's choice; experiments)
CONV_DGRAD_TILE = 0


# the data gradient over a zero-padded copy of the output gradient (F.pad: a fill and a copy per
# layer) instead of the bounded loader
CONV_DGRAD_PAD_COPY = False


def conv_x6_u8_ok(src, weight, stride: int, B: int, wgrad: bool = False) -> bool:
    """The first convolution straight from u8 frame stacks src [R, C, H, W] (ocppo_conv_x6_u8):
    KW, W and the stride multiples of 4, no padding, B samples' rows a tile divides."""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and
            src.dim() == 4 and src.is_contiguous() and weight.dim() == 4):
        return False
    _, C, H, W = src.shape
    Cout, Cw, KH, KW = weight.shape
    s = int(stride)
    if Cw != C or KW % 4 or W % 4 or s % 4 or H < KH or W < KW or (H - KH) % s or (W - KW) % s:
        return False
    OH, OW = (H - KH) // s + 1, (W - KW) // s + 1
    rows, taps = B * OH * OW, C * KH * KW
    if rows >= 1 << 24 or taps % 32 or taps // 4 > 1024 or _conv_u8_tile(rows, Cout, 0) is None:
        return False
    return not wgrad or (OH * OW <= 1024 and rows % 32 == 0 and
                         _conv_u8_tile(Cout, taps, 1) is not None)


def _conv_u8_tile(M: int, N: int, mode: int) -> int | None:
    for t in (((0,) if N == 32 else (2,) if N == 64 else ()) if mode == 0 else
              ((1,) if M == 32 else (4,) if M == 64 else ())):
        bm, bn = _CONV_TILES[t]
        if M % bm == 0 and N % bn == 0:
            return t
    return None


# The first convolution's forward with each image's u8 stack staged in LDS once (ocppo_conv_x6_u8
# tile 7, conv_u8_img_kernel: bitwise the tile loop's output) where the geometry is NatureCNN's
# first layer (4 x 84 x 84 stacks, 8 x 8 taps, stride 4, 32 channels)
CONV_U8_IMG = True


def _conv_u8_img_ok(src, weight, stride: int) -> bool:
    _, C, H, W = src.shape
    Cout, _, KH, KW = weight.shape
    OH, OW = (H - KH) // stride + 1, (W - KW) // stride + 1
    return (CONV_U8_IMG and C == 4 and KH == 8 and KW == 8 and stride == 4 and Cout == 32 and
            (OH * OW) % 16 == 0 and (C * H * W) % 16 == 0 and 2 * C * H * W <= 65536 and
            src.data_ptr() % 16 == 0)


def conv_x6_u8(src, idx, weight, bias=None, stride: int = 4, relu: bool = True,
               divisor: float = 255.0, out=None, tile: int | None = None, mbits=None,
               wn=None):
    """act(conv2d(src[idx] / divisor, weight) + bias) with the u8 frame stacks read in place
    (ocppo_conv_x6_u8): src [R, C, H, W] u8, idx [B] int64 -> channels_last [B, Cout, OH, OW].
    tile: None = the image-staged kernel where it applies (CONV_U8_IMG), else the tile loop's;
    an explicit ocppo_conv_x6_u8 tile forces that form (tests). mbits: an int32 [B OH OW] tensor
    the image-staged kernel fills with the output's ReLU mask (bit co of row r = out > 0), for
    conv_x6_u8_wgrad's fused ReLU backward. wn: the weight already in nn.Conv2d's contiguous
    (c, ky, kx) tap order (a cached copy of a channels_last weight), else made here."""
    B = idx.numel()
    if not conv_x6_u8_ok(src, weight, stride, B):
        raise ValueError(f"conv_x6_u8: unsupported src {tuple(src.shape)} / weight "
                         f"{tuple(weight.shape)} / stride {stride} / {B} samples")
    _, C, H, W = src.shape
    Cout, _, KH, KW = weight.shape
    s = int(stride)
    OH, OW = (H - KH) // s + 1, (W - KW) // s + 1
    dev, f = src.device, torch.float32
    K, M = C * KH * KW, B * OH * OW
    if wn is None:
        wn = weight.contiguous()  # nn.Conv2d's (c, ky, kx) tap order
    elif tuple(wn.shape) != tuple(weight.shape) or not wn.is_contiguous():
        raise ValueError("conv_x6_u8: wn must be the weight as a contiguous tensor")
    if out is None:
        out = torch.empty((B, Cout, OH, OW), dtype=f, device=dev, memory_format=torch.channels_last)
    if tuple(out.shape) != (B, Cout, OH, OW) or not out.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("conv_x6_u8: out must be a channels_last [B, Cout, OH, OW] tensor")
    _bounds(dev, u8=src)
    if tile is None:
        tile = 7 if _conv_u8_img_ok(src, weight, s) else _conv_u8_tile(M, Cout, 0)
    if mbits is not None and (tile != 7 or not relu):
        raise ValueError("conv_x6_u8: mbits needs the image-staged kernel (tile 7) and relu")
    call("ocppo_conv_x6_u8", _stream(dev), 0, src.data_ptr(), _check(idx, "idx", torch.int64, dev, B),
         C, H, W, KH, KW, s, wn.data_ptr(), K, out.data_ptr(), M, Cout, K, 1,
         _opt(bias, "bias", f, dev, Cout), int(bool(relu)), float(divisor), tile, None,
         _opt(mbits, "mbits", torch.int32, dev, M), None, None)
    return out


# ... and its weight gradient (ocppo_conv_x6_u8 tile 8, conv_u8_wgrad_img_kernel: each image's
# stack in LDS once, rewritten per channel as tap-column rows; 4 partials per workgroup summed in
# order) for NatureCNN's first layer on 4 x 84 x 84 stacks
CONV_U8_IMG_WGRAD = True


@functools.lru_cache(maxsize=None)
def _cus(dev) -> int:
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _conv_u8_img_wgrad_ok(src, kernel, stride: int, Cout: int) -> bool:
    _, C, H, W = src.shape
    return (CONV_U8_IMG_WGRAD and C == 4 and H == 84 and W == 84 and tuple(kernel) == (8, 8) and
            stride == 4 and Cout == 32 and src.data_ptr() % 16 == 0)


def conv_x6_u8_wgrad(gp, src, idx, kernel: tuple, stride: int = 4, divisor: float = 255.0,
                     out=None, tile: int | None = None, mbits=None, db=None):
    """dW [Cout, C KH KW] (nn.Conv2d's tap order) of conv_x6_u8: sum over the output pixels r of
    gp[r, co] src[idx[b], c, s oy + ky, s ox + kx] / divisor; split partials summed in order.
    tile: None = the image-staged kernel where it applies (CONV_U8_IMG_WGRAD), else the tile
    loop's; an explicit ocppo_conv_x6_u8 tile forces that form (tests). Image-staged kernel only:
    mbits (conv_x6_u8's ReLU mask) makes gp the UNMASKED output gradient, masked in the kernel
    (relu_bias_grad's ReLU backward); db [Cout] receives the masked gradient's column sums (the
    bias gradient)."""
    B = idx.numel()
    _, C, H, W = src.shape
    KH, KW = kernel
    s = int(stride)
    OH, OW = (H - KH) // s + 1, (W - KW) // s + 1
    rows, Cout = gp.shape
    dev, f = src.device, torch.float32
    N = C * KH * KW
    if tile is None and _conv_u8_img_wgrad_ok(src, kernel, s, Cout):
        tile = 8
    if (mbits is not None or db is not None) and tile != 8:
        raise ValueError("conv_x6_u8_wgrad: mbits / db need the image-staged kernel (tile 8)")
    if tile == 8:
        if rows != B * OH * OW:
            raise ValueError("conv_x6_u8_wgrad: gp must be [B OH OW, Cout]")
        S = 4 * min(_cus(dev), B)  # 4 wave partials per workgroup, <= one workgroup per image
        part = _persistent("conv_x6_u8_wgrad.img", dev, (S, Cout, N),
                           lambda: torch.empty((S, Cout, N), dtype=f, device=dev))
        if out is None:
            out = torch.empty((Cout, N), dtype=f, device=dev)
        dbp = None
        if db is not None:
            dbp = _persistent("conv_x6_u8_wgrad.img_db", dev, (S, Cout),
                              lambda: torch.empty((S, Cout), dtype=f, device=dev)).data_ptr()
        _bounds(dev, u8=src)
        call("ocppo_conv_x6_u8", _stream(dev), 1, src.data_ptr(),
             _check(idx, "idx", torch.int64, dev, B), C, H, W, KH, KW, s,
             _check(gp, "gp", f, dev), Cout, part.data_ptr(), Cout, N, rows, S, None, 0,
             float(divisor), 8, _check(out, "out", f, dev, Cout * N),
             _opt(mbits, "mbits", torch.int32, dev, rows), dbp, _opt(db, "db", f, dev, Cout))
        return out
    tile = _conv_u8_tile(Cout, N, 1) if tile is None else tile
    if rows != B * OH * OW or tile is None or rows % 32:
        raise ValueError("conv_x6_u8_wgrad: gp must be [B OH OW, Cout] with a tile for it")
    bm, bn = _CONV_TILES[tile]
    S = max(1, min(rows // 32 // 32, _wgrad_units(tile) // ((Cout // bm) * (N // bn))))
    part = _persistent("conv_x6_u8_wgrad", dev, (S, Cout, N),
                       lambda: torch.empty((S, Cout, N), dtype=f, device=dev))
    if out is None:
        out = torch.empty((Cout, N), dtype=f, device=dev)
    _bounds(dev, u8=src)
    call("ocppo_conv_x6_u8", _stream(dev), 1, src.data_ptr(), _check(idx, "idx", torch.int64, dev, B),
         C, H, W, KH, KW, s, _check(gp, "gp", f, dev), Cout, part.data_ptr(), Cout, N, rows, S,
         None, 0, float(divisor), tile, _check(out, "out", f, dev, Cout * N), None, None, None)
    return out


def linear2_act(x, w1, b1, w2, b2, relu1: bool = True, relu2: bool = True, out=None):
    """y = act2(act1(x @ w1.T + b1) @ w2.T + b2) in ONE launch for rollout-sized batches (no
    autograd): x [M, K1] f32 (unit column stride, K1 <= 64), w1 [N1, K1], w2 [N2, N1]
    (N1 % 16 == 0, N1 <= 512)."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be [M, K1] with unit column stride")
    M, K1 = x.shape
    N1, N2 = w1.shape[0], w2.shape[0]
    if w1.shape[1] != K1 or w2.shape[1] != N1:
        raise ValueError(f"shapes: x {tuple(x.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}")
    dev = x.device
    f = torch.float32
    if out is None:
        out = torch.empty((M, N2), dtype=f, device=dev)
    if x.dtype != f or x.device.type != "cuda":
        raise ValueError("x must be a float32 GPU tensor")
    call("ocppo_linear2_act", _stream(dev), x.data_ptr(), x.stride(0) if M > 1 else K1,
         _check(w1, "w1", f, dev), _opt(b1, "b1", f, dev, N1), _check(w2, "w2", f, dev),
         _opt(b2, "b2", f, dev, N2), _check(out, "out", f, dev, M * N2), N2, M, N1, N2, K1,
         int(bool(relu1)), int(bool(relu2)))
    return out


def linear_cache_shift(x, weight, bias, enc, done=None, relu: bool = True):
    """The rollout's last encoder layer and the frame-encoding cache shift in one launch:
    fresh = act(x @ weight.T + bias) (x [M, K] f32, unit column stride; weight [E, K]) shifts
    enc [M, W, E] like ops.frame_cache_shift(enc, fresh, done) without storing fresh."""
    if x.dim() != 2 or weight.dim() != 2 or enc.dim() != 3:
        raise ValueError(f"x [M, K], weight [E, K], enc [M, W, E] expected, got {tuple(x.shape)}, "
                         f"{tuple(weight.shape)}, {tuple(enc.shape)}")
    M, K = x.shape
    E = weight.shape[0]
    dev = x.device
    if weight.shape[1] != K or enc.shape[0] != M or enc.shape[2] != E:
        raise ValueError(f"shapes: x {tuple(x.shape)}, weight {tuple(weight.shape)}, "
                         f"enc {tuple(enc.shape)}")
    if x.dtype != torch.float32 or (M > 1 and x.stride(1) != 1) or x.device.type != "cuda":
        raise ValueError("x must be an f32 GPU tensor with unit column stride")
    call("ocppo_linear_cache_shift", _stream(dev), x.data_ptr(), x.stride(0) if M > 1 else K,
         _check(weight, "weight", torch.float32, dev), _opt(bias, "bias", torch.float32, dev, E),
         _check(enc, "enc", torch.float32, dev), _opt(done, "done", torch.float32, dev, M), M, E,
         K, enc.shape[1], 1 if relu else 0)
    return enc


def linear_cache_ring(x, weight, bias, enc, slot: int, done=None, relu: bool = True):
    """The rollout's last encoder layer writing the frame-encoding RING: fresh = act(x @ weight.T
    + bias) overwrites physical slot `slot` of enc [M, W, E] (every slot of an env with
    done != 0); nothing is shifted (ocppo_linear_cache_ring; read back with
    linear_act(..., ring=(E, rot)))."""
    if x.dim() != 2 or weight.dim() != 2 or enc.dim() != 3:
        raise ValueError(f"x [M, K], weight [E, K], enc [M, W, E] expected, got {tuple(x.shape)}, "
                         f"{tuple(weight.shape)}, {tuple(enc.shape)}")
    M, K = x.shape
    E = weight.shape[0]
    dev = x.device
    if weight.shape[1] != K or enc.shape[0] != M or enc.shape[2] != E:
        raise ValueError(f"shapes: x {tuple(x.shape)}, weight {tuple(weight.shape)}, "
                         f"enc {tuple(enc.shape)}")
    if x.dtype != torch.float32 or (M > 1 and x.stride(1) != 1) or x.device.type != "cuda":
        raise ValueError("x must be an f32 GPU tensor with unit column stride")
    call("ocppo_linear_cache_ring", _stream(dev), x.data_ptr(), x.stride(0) if M > 1 else K,
         _check(weight, "weight", torch.float32, dev), _opt(bias, "bias", torch.float32, dev, E),
         _check(enc, "enc", torch.float32, dev), _opt(done, "done", torch.float32, dev, M), M, E,
         K, enc.shape[1], int(slot), 1 if relu else 0)
    return enc


def store_linear2(frame, reward, done, prev_obs, obs_out, net_obs, done_out, reward_out, w1, b1,
                  w2, b2, y, vecnorm_state=None, gamma=0.99, epsilon=1e-8, clip_reward=10.0):
    """ONE launch: the rollout store of the previous step (ops.rollout_store, or
    ops.rollout_store_vecnorm when vecnorm_state = (ret_state, rms_state)) and
    y = relu(relu(f @ w1.T + b1) @ w2.T + b2) of the newest frames f (frame seen through the
    storage dtype of obs_out, f32 or bf16). frame [N, D] f32, obs [N, W, D], net_obs [N, W, D]
    f32, y [N, N2] f32 (row stride may exceed N2)."""
    N, D = frame.shape
    W = obs_out.shape[1]
    dev = frame.device
    f = torch.float32
    if frame.dtype != f:
        raise ValueError("store_linear2: object frames only (f32)")
    if prev_obs.shape != obs_out.shape or prev_obs.dtype != obs_out.dtype or \
            tuple(obs_out.shape) != (N, W, D) or obs_out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"obs slots must be [N, W, D] f32|bf16, got {tuple(obs_out.shape)} "
                         f"{obs_out.dtype}")
    N1, N2 = w1.shape[0], w2.shape[0]
    if tuple(w1.shape) != (N1, D) or tuple(w2.shape) != (N2, N1) or y.shape[0] != N or \
            y.shape[1] != N2 or y.stride(1) != 1 or y.dtype != f:
        raise ValueError(f"shapes: frame {tuple(frame.shape)}, w1 {tuple(w1.shape)}, "
                         f"w2 {tuple(w2.shape)}, y {tuple(y.shape)}")
    vn = vecnorm_state is not None
    ret, rms = vecnorm_state if vn else (None, None)
    call("ocppo_store_linear2", _stream(dev), _check(frame, "frame", f, dev),
         _check(reward, "reward", f, dev, N), _check(done, "done", f, dev, N), N, W, D,
         _check(prev_obs, "prev_obs", None, dev), _check(obs_out, "obs_out", None, dev),
         _DTYPE_CODE[obs_out.dtype], _opt(net_obs, "net_obs", f, dev, N * W * D),
         _check(reward_out, "reward_out", f, dev, N), _opt(done_out, "done_out", f, dev, N),
         int(vn), float(gamma), float(epsilon), float(clip_reward),
         _opt(ret, "ret_state", torch.float64, dev, N), _opt(rms, "rms_state", torch.float64, dev, 3),
         _check(w1, "w1", f, dev), _opt(b1, "b1", f, dev, N1), _check(w2, "w2", f, dev),
         _opt(b2, "b2", f, dev, N2), y.data_ptr(), y.stride(0) if N > 1 else N2, N1, N2)
    return y


def head_env_store_linear2_ok(hidden, w_actor, w_critic, env) -> bool:
    """head_env_store_linear2 applies: policy_head_env_step's conditions with H = 256 or 512."""
    return policy_head_env_ok(hidden, w_actor, w_critic, env) and hidden.shape[1] in (256, 512) \
        and env.frame.shape[1] <= 64


def head_env_store_linear2(hidden, w_actor, b_actor, w_critic, b_critic, noise, action_out,
                           logprob_out, value_out, env, step_offset: int, prev_obs, obs_out,
                           net_obs, done_out, reward_out, w1, b1, w2, b2, y, vecnorm_state=None,
                           gamma=0.99, epsilon=1e-8, clip_reward=10.0):
    """ONE launch: policy_head_env_step(hidden, ..., env, step_offset) followed by
    store_linear2(env.frame, env.reward, env.done, prev_obs, obs_out, ...) -- the head, sample
    and env step of one rollout step, its store, and the next step's first two encoder layers
    (ocppo_head_env_store_linear2; bitwise the two launches). noise [N, A] is read."""
    N, H = hidden.shape
    A = w_actor.shape[0]
    D = env.frame.shape[1]
    W = obs_out.shape[1]
    dev = hidden.device
    f = torch.float32
    if tuple(w_actor.shape) != (A, H) or w_critic.numel() != H or b_actor.numel() != A:
        raise ValueError("head weights do not match hidden")
    if prev_obs.shape != obs_out.shape or prev_obs.dtype != obs_out.dtype or \
            tuple(obs_out.shape) != (N, W, D) or obs_out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"obs slots must be [N, W, D] f32|bf16, got {tuple(obs_out.shape)} "
                         f"{obs_out.dtype}")
    N1, N2 = w1.shape[0], w2.shape[0]
    if tuple(w1.shape) != (N1, D) or tuple(w2.shape) != (N2, N1) or y.shape[0] != N or \
            y.shape[1] != N2 or y.stride(1) != 1 or y.dtype != f:
        raise ValueError(f"shapes: frame {tuple(env.frame.shape)}, w1 {tuple(w1.shape)}, "
                         f"w2 {tuple(w2.shape)}, y {tuple(y.shape)}")
    vn = vecnorm_state is not None
    ret, rms = vecnorm_state if vn else (None, None)
    call("ocppo_head_env_store_linear2", _stream(dev), _check(hidden, "hidden", f, dev), H,
         _check(w_actor, "w_actor", f, dev), _check(b_actor, "b_actor", f, dev, A),
         _check(w_critic, "w_critic", f, dev, H), _check(b_critic, "b_critic", f, dev, 1),
         _check(noise, "noise", f, dev, N * A), A,
         _check(action_out, "action_out", torch.int64, dev, N),
         _check(logprob_out, "logprob_out", f, dev, N), _check(value_out, "value_out", f, dev, N),
         env.seed & 0xFFFFFFFFFFFFFFFF, _check(env.step_base, "step_base", torch.int64, dev, 1),
         int(step_offset), _check(env.frame, "frame", f, dev, N * D),
         _check(env.reward, "reward", f, dev, N), _check(env.done, "done", f, dev, N),
         _opt(env.ep_state, "ep_state", f, dev, N * 5), N, W, D,
         _check(prev_obs, "prev_obs", None, dev), _check(obs_out, "obs_out", None, dev),
         _DTYPE_CODE[obs_out.dtype], _opt(net_obs, "net_obs", f, dev, N * W * D),
         _check(reward_out, "reward_out", f, dev, N), _opt(done_out, "done_out", f, dev, N),
         int(vn), float(gamma), float(epsilon), float(clip_reward),
         _opt(ret, "ret_state", torch.float64, dev, N), _opt(rms, "rms_state", torch.float64, dev, 3),
         _check(w1, "w1", f, dev), _opt(b1, "b1", f, dev, N1), _check(w2, "w2", f, dev),
         _opt(b2, "b2", f, dev, N2), y.data_ptr(), y.stride(0) if N > 1 else N2, N1, N2)
    return y


# ---------------------------------------------------------------------------------------------
# Linear(+ReLU) backward, elementwise part: threshold_backward + bias sum in one pass
# (autograd of architectures/ppo.py:60-84 inside ppo_atari_oc.py:605)
# ---------------------------------------------------------------------------------------------
def _relu_bias_ws(R: int, N: int, dev):
    """relu_bias_grad's tickets (zeroed once, then self re-arming)."""
    return _persistent("relu_bias_grad", dev, (R, N), lambda: torch.zeros(
        int(_lib.LIB.ocppo_relu_bias_grad_workspace_bytes(R, N)), dtype=torch.uint8, device=dev))


def relu_bias_grad_ok(g) -> bool:
    return (g.is_cuda and g.dtype == torch.float32 and g.dim() == 2 and g.shape[1] % 4 == 0
            and 4 <= g.shape[1] <= 16384 and g.is_contiguous() and g.data_ptr() % 16 == 0)


def relu_bias_grad(g, out=None, db=None, gp=None, bits=None):
    """(gp, db): gp = threshold_backward(g, out, 0) (g itself when out is None), db = gp.sum(0),
    in one pass over g [R, N] f32 (N % 4 == 0). Deterministic. bits: the ReLU mask as the
    forward epilogue's row-major bitmask (int32 [R N / 32], conv_x6(..., mbits=)) instead of out."""
    if g.dim() != 2:
        raise ValueError(f"g must be [R, N], got {tuple(g.shape)}")
    R, N = g.shape
    dev = g.device
    f = torch.float32
    if db is None:
        db = torch.empty(N, dtype=f, device=dev)
    if bits is not None:
        gp = torch.empty_like(g) if gp is None else gp
        ws = _relu_bias_ws(R, N, dev)
        call("ocppo_relu_bias_grad_bits", _stream(dev), _check(g, "g", f, dev),
             _check(bits, "bits", torch.int32, dev, R * N // 32), _check(gp, "gp", f, dev, R * N),
             _check(db, "db", f, dev, N), R, N, ws.data_ptr(), ws.numel())
        return gp, db
    if out is not None and gp is None:
        gp = torch.empty_like(g)
    ws = _relu_bias_ws(R, N, dev)
    call("ocppo_relu_bias_grad", _stream(dev), _check(g, "g", f, dev),
         _opt(out, "out", f, dev, R * N), _opt(gp, "gp", f, dev, R * N),
         _check(db, "db", f, dev, N), R, N, ws.data_ptr(), ws.numel())
    return (gp if out is not None else g), db


def relu_bias_grad_partial(g, out=None, gp=None):
    """(gp, (partials, chunks)): relu_bias_grad with the bias-gradient chunk sums left for
    sum_splits_db (deferred to the launch that combines the layer's split-K weight gradient).
    partials [chunks, N] f32 is a per-shape persistent buffer (_persistent)."""
    R, N = g.shape
    dev = g.device
    f = torch.float32
    if out is not None and gp is None:
        gp = torch.empty_like(g)
    def make():
        chunks = int(_lib.LIB.ocppo_relu_bias_grad_chunks(R, N))
        return torch.zeros((chunks, N), dtype=f, device=dev), chunks

    buf = _persistent("relu_bias_grad_partial", dev, (R, N), make)
    call("ocppo_relu_bias_grad_partial", _stream(dev), _check(g, "g", f, dev),
         _opt(out, "out", f, dev, R * N), _opt(gp, "gp", f, dev, R * N), buf[0].data_ptr(), R, N)
    return (gp if out is not None else g), buf


def sum_splits_db(part, out, db_part, db, finish=None):
    """sum_splits(part, out) and db = db_part.sum(0) in a fixed order, one launch
    (db_part = the (partials, chunks) of relu_bias_grad_partial). finish = a filled
    DeferredFinish of relu_bias_wgrad(..., defer=): run by extra workgroups of the same launch
    (ocppo_sum_splits_db_finish; out / db bitwise the same)."""
    S = part.shape[0]
    dev = part.device
    f = torch.float32
    parts, chunks = db_part
    N = parts.shape[1]
    n = part[0].numel()
    args = (_check(part, "part", f, dev), S, n, _check(out, "out", f, dev, n),
            _check(parts, "db_partials", f, dev, chunks * N), chunks, N,
            _check(db, "db", f, dev, N))
    if finish is not None and finish.filled:
        finish.pending = False
        call("ocppo_sum_splits_db_finish", _stream(dev), *args, finish.ptr())
    else:
        call("ocppo_sum_splits_db", _stream(dev), *args)
    return out, db


def relu_bias_wgrad_ok(g, x) -> bool:
    return (relu_bias_grad_ok(g) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
            and 1 <= x.shape[1] <= 16 and x.shape[0] == g.shape[0] and x.stride(1) == 1)


def relu_bias_wgrad(g, out, x, dw=None, db=None, defer=None):
    """(dw, db) of a Linear(+ReLU) layer whose input needs no gradient, in one pass:
    gp = threshold_backward(g, out, 0) (g when out is None, never materialised),
    db = gp.sum(0), dw = gp^T x. g [R, N] f32 (N % 4 == 0), x [R, K] f32 (K <= 16).
    defer = a DeferredFinish (R >= 1): only the rows launch runs now (ocppo_relu_bias_wgrad_rows);
    dw and db are written when the caller runs the finish (sum_splits_db(..., finish=) or run())."""
    if g.dim() != 2 or x.dim() != 2 or x.shape[0] != g.shape[0]:
        raise ValueError(f"g [R, N] and x [R, K] expected, got {tuple(g.shape)}, {tuple(x.shape)}")
    R, N = g.shape
    K = x.shape[1]
    dev = g.device
    f = torch.float32
    if x.stride(1) != 1 and R > 0:
        raise ValueError("x must have unit column stride")
    ldx = x.stride(0) if R > 1 else K
    if dw is None:
        dw = torch.empty((N, K), dtype=f, device=dev)
    if db is None:
        db = torch.empty(N, dtype=f, device=dev)
    if tuple(dw.shape) != (N, K) or not dw.is_contiguous():
        raise ValueError(f"dw must be a contiguous [{N}, {K}] tensor")
    ws = _persistent("relu_bias_wgrad", dev, (R, N, K), lambda: torch.zeros(
        int(_lib.LIB.ocppo_relu_bias_wgrad_workspace_bytes(R, N, K)), dtype=torch.uint8,
        device=dev))
    call("ocppo_relu_bias_wgrad_rows" if defer is not None else "ocppo_relu_bias_wgrad",
         _stream(dev), _check(g, "g", f, dev),
         _opt(out, "out", f, dev, R * N),
         _check(x, "x", f, dev) if x.is_contiguous() else x.data_ptr(), ldx,
         _check(dw, "dw", f, dev, N * K), _check(db, "db", f, dev, N), R, N, K, ws.data_ptr(),
         ws.numel(), *((defer.ptr(),) if defer is not None else ()))
    if defer is not None:
        defer.pending = defer.filled = True
    return dw, db


def heads_bwd_ok(h, A: int) -> bool:
    return (h.is_cuda and h.dtype == torch.float32 and h.dim() == 2 and h.shape[0] >= 1 and
            h.shape[1] % 4 == 0 and 4 <= h.shape[1] <= 16384 and 1 <= A <= 7 and
            h.is_contiguous() and h.data_ptr() % 16 == 0)


def heads_bwd(h, dlogits, dvalue, wa, wc, relu: bool = True, gp=None, db_h=None, dwa=None,
              dwc=None, dba=None, dbc=None):
    """Actor/critic heads' backward + the producing layer's ReLU backward in one pass (see
    include/ocppo.h). h [M, H] (the heads' input = decoder ReLU output), dlogits [M, A],
    dvalue [M]; returns (gp, db_h, dwa, dwc, dba, dbc); db_h None skips the decoder bias.
    dvalue = wc = None: a single head (dwc, dbc returned as None)."""
    M, H = h.shape
    A = dlogits.shape[1]
    dev = h.device
    f = torch.float32
    critic = wc is not None
    if critic != (dvalue is not None):
        raise ValueError("dvalue and wc: both or neither")
    gp = torch.empty_like(h) if gp is None else gp
    dwa = torch.empty(A, H, dtype=f, device=dev) if dwa is None else dwa
    dba = torch.empty(A, dtype=f, device=dev) if dba is None else dba
    if critic:
        dwc = torch.empty(1, H, dtype=f, device=dev) if dwc is None else dwc
        dbc = torch.empty(1, dtype=f, device=dev) if dbc is None else dbc
    else:
        dwc = dbc = None
    ws = _persistent("heads_bwd", dev, (M, H, A), lambda: torch.zeros(
        int(_lib.LIB.ocppo_heads_bwd_workspace_bytes(M, H, A)), dtype=torch.uint8, device=dev))
    call("ocppo_heads_bwd", _stream(dev), _check(h, "h", f, dev, M * H),
         _check(dlogits, "dlogits", f, dev, M * A), _opt(dvalue, "dvalue", f, dev, M),
         _check(wa, "wa", f, dev, A * H), _opt(wc, "wc", f, dev, H),
         _check(gp, "gp", f, dev, M * H), _opt(db_h, "db_h", f, dev, H),
         _check(dwa, "dwa", f, dev, A * H), _opt(dwc, "dwc", f, dev, H),
         _check(dba, "dba", f, dev, A), _opt(dbc, "dbc", f, dev, 1), M, H, A,
         1 if relu else 0, ws.data_ptr(), ws.numel())
    return gp, db_h, dwa, dwc, dba, dbc


def bias_act(y, b, relu: bool = True):
    """In place: y = act(y + b) over the rows of y [R, N] f32 (N % 4 == 0): the bias add + ReLU
    after a bias-less convolution (NHWC output viewed [B*H*W, C]) in one pass."""
    if y.dim() != 2:
        raise ValueError(f"y must be [R, N], got {tuple(y.shape)}")
    R, N = y.shape
    dev = y.device
    call("ocppo_bias_act", _stream(dev), _check(y, "y", torch.float32, dev),
         _check(b, "b", torch.float32, dev, N), R, N, int(bool(relu)))
    return y


def bias_act_nchw(y, b, relu: bool = True, out=None):
    """act(y + b) of a channels_last conv output y [B, C, H, W] (bias-less), returned as an
    NCHW-contiguous tensor (so an nn.Flatten after it is a view): one pass, layout copy included."""
    if y.dim() != 4 or not y.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("y must be a channels_last [B, C, H, W] tensor")
    B, C, H, W = y.shape
    dev = y.device
    f = torch.float32
    if out is None:
        out = torch.empty((B, C, H, W), dtype=f, device=dev)
    if not out.is_contiguous() or tuple(out.shape) != (B, C, H, W):
        raise ValueError("out must be a contiguous (NCHW) [B, C, H, W] tensor")
    call("ocppo_bias_act_nchw", _stream(dev), _check(y.permute(0, 2, 3, 1), "y", f, dev),
         _check(b, "b", f, dev, C),
         B, H * W, C, int(bool(relu)), _check(out, "out", f, dev, B * C * H * W))
    return out


def sum_splits_ok(part, out) -> bool:
    return (part.is_cuda and part.dtype == torch.float32 and part.is_contiguous() and
            out.is_contiguous() and out.dtype == torch.float32 and part.shape[0] in (1, 2, 4, 8, 16)
            and part[0].numel() % 4 == 0 and part.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0)


def sum_splits(part, out=None, finish=None):
    """out = part.sum(0) over the S split-K partial blocks of a weight gradient, in split order
    (added in f64, rounded once), in one streaming pass (part [S, ...] f32 contiguous, S in {1, 2, 4, 8, 16}).
    finish = a filled DeferredFinish: run by extra workgroups of the same launch
    (ocppo_sum_splits_finish; out bitwise the same)."""
    S = part.shape[0]
    dev = part.device
    if out is None:
        out = torch.empty(part.shape[1:], dtype=torch.float32, device=dev)
    n = part[0].numel()
    if finish is not None and finish.filled:
        finish.pending = False
        call("ocppo_sum_splits_finish", _stream(dev), _check(part, "part", torch.float32, dev), S,
             n, _check(out, "out", torch.float32, dev, n), finish.ptr())
        return out
    call("ocppo_sum_splits", _stream(dev), _check(part, "part", torch.float32, dev), S, n,
         _check(out, "out", torch.float32, dev, n))
    return out


# ---------------------------------------------------------------------------------------------
# Update-phase f32 GEMMs on the bf16 matrix cores (ocppo_gemm_x6; ppo_atari_oc.py:566-606)
# ---------------------------------------------------------------------------------------------
# (rows, columns) of variant & 7 (0-3: 4 waves, 4-7: 8 waves); variant & 8: loads two K steps
# ahead; variant & 16: one accumulator (built: every shape with both, shapes 0-3 with neither or
# only the latter). Variant 56: mixed tiles — rows [0, mbig) in 128 x 128 tiles dispatched first,
# the rest in 64 x 128 (mbig chosen in the library, include/ocppo.h); it divides, and counts its
# dbp rows and mask words, like 64 x 128
X6_TILES = ((128, 128), (64, 128), (128, 64), (64, 64),
            (128, 128), (64, 128), (128, 128), (128, 64)) * 7 + ((64, 128),) + (
    (256, 128), (128, 256), (128, 128), (128, 128)) + ((0, 0),) * 3
# workgroup threads of each variant (the ReLU bitmask holds one 64-bit word per thread and tile)
X6_THREADS = (256,) * 4 + (512,) * 4
X6_BUILT = tuple(range(4)) + tuple(range(16, 20)) + tuple(range(24, 32)) + (56, 57, 58, 59, 60)
X6_MIXED = 56
# the pipelined family (ocppo_gemm.hip gemm_x6p_kernel): two LDS stages, one barrier per K step
X6_PIPE = (57, 58, 59, 60)
X6_PIPE_THREADS = {57: 512, 58: 512, 59: 256, 60: 512}


X6_AUTO = 24  # the variant family x6_tile picks from (two K steps of loads in flight, one
# accumulator: fastest at every config-2 update shape, tools/exp_gemm_x6.py; error vs f64 at or
# below hipBLASLt's f32 GEMM, tests/test_gemm_gpu.py)


def x6_tile(M: int, N: int, splits: int = 1, tile: int | None = None) -> int | None:
    """Tile for an M x N (x splits) product: the largest tile that divides it and still gives
    >= 256 workgroups (one per CU; 128 x 128 is the fastest at every config-2 shape that has
    that many, tools/exp_gemm_x6.py), else the one giving the most; None if none divides."""
    if tile is not None:
        if tile not in X6_BUILT:
            return None  # no such variant in the library
        bm, bn = X6_TILES[tile]
        if tile == X6_MIXED and splits != 1:
            return None
        return tile if M % bm == 0 and N % bn == 0 else None
    # 256 < tiles of 128 x 128 <= 384 (more than one per CU, fewer than two): the mixed variant,
    # one 128 x 128 tile per CU and the rest in 64 x 128 tiles beside them (tools/exp_gemm_x6.py
    # --mbig; the split itself is chosen in the library)
    t128 = (M // 128) * (N // 128)
    if (splits == 1 and M % 128 == 0 and N % 128 == 0 and 256 < t128 <= 384
            and 256 % (N // 128) == 0):
        return X6_MIXED
    best, best_units = None, -1
    for i, (bm, bn) in enumerate(X6_TILES[:4]):
        i += X6_AUTO
        if M % bm or N % bn:
            continue
        units = splits * (M // bm) * (N // bn)
        if units >= 256:
            return i
        if units > best_units:
            best, best_units = i, units
    return best


def _x6_operand_ok(t) -> bool:
    return (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.data_ptr() % 16 == 0
            and t.stride(1) == 1 and t.stride(0) % 4 == 0)


def x6_sk_workspace(tile: int, device):
    """The stream-K workspace of a pipelined tile on `device` (zeroed once; every launch leaves
    its flags at zero again)."""
    def make():
        n = _lib.LIB.ocppo_gemm_x6_sk_workspace_bytes(tile)
        if n == 0:
            raise ValueError(f"gemm_x6: tile {tile} has no stream-K form")
        return torch.zeros(n, dtype=torch.uint8, device=device)

    return _persistent("x6_sk_workspace", device, tile, make)


def x6_mbits_words(M: int, N: int, tile: int) -> int:
    """64-bit words of a gemm_x6 ReLU bitmask over an [M, N] output with `tile`."""
    bm, bn = X6_TILES[tile]
    nt = X6_PIPE_THREADS[tile] if tile in X6_PIPE_THREADS else X6_THREADS[tile & 7]
    return (M // bm) * (N // bn) * nt


def gemm_x6(a, sam, sak, b, sbn, sbk, c, ldc, M, N, K, splits=1, split_c=0, bias=None,
            relu=False, mask=None, dbp=None, tile=None, mbits_out=None, mbits_in=None, mbig=None,
            b_planes=None, stream_k=False, mbits_rows=False):
    """Raw ocppo_gemm_x6 call on tensors a, b, c (their data pointers; strides as given).
    mbig: rows in 128 x 128 tiles for the mixed variant (None: the library's choice).
    b_planes: B pre-split, bf16 [3, N, K] (split_planes of B); b may then be None.
    stream_k: a pipelined tile (57 / 58) as a persistent stream-K launch (x6_sk_workspace)."""
    t = x6_tile(M, N, splits, tile)
    if t is None:
        raise ValueError(f"gemm_x6: no tile divides {M} x {N}")
    dev = c.device
    if b_planes is not None:
        if (b_planes.dtype != torch.bfloat16 or tuple(b_planes.shape) != (3, N, K)
                or not b_planes.is_contiguous() or b_planes.device != dev or sak != 1
                or K % 8 or not (X6_AUTO <= t < X6_AUTO + 4 or t in (X6_MIXED, 57, 58))):
            raise ValueError("gemm_x6: b_planes must be a contiguous bf16 [3, N, K] on the "
                             "output's device, with a k-contiguous A and a tile of the x6 family")
    if mask is not None:
        if (mask.dim() != 2 or tuple(mask.shape) != (M, N) or mask.stride(1) != 1
                or mask.dtype != torch.float32 or dbp is None):
            raise ValueError("gemm_x6: mask must be an f32 [M, N] row-major view, with dbp")
    if mask is not None or mbits_in is not None:
        _check(dbp, "dbp", torch.float32, dev, (M // X6_TILES[t][0]) * N)
    if mbits_rows:
        if not relu or mbits_out is None:
            raise ValueError("gemm_x6: the row-major bitmask needs relu and mbits_out")
        _check(mbits_out, "mbits", torch.int32, dev, M * N // 32)
    for mb in ((mbits_in,) if mbits_rows else (mbits_out, mbits_in)):
        if mb is not None:
            _check(mb, "mbits", torch.int64, dev, x6_mbits_words(M, N, t))
    bp = None if bias is None else _check(bias, "bias", torch.float32, dev, N)
    args = (a.data_ptr(), sam, sak, None if b is None else b.data_ptr(), sbn, sbk, c.data_ptr(),
            ldc, M, N, K, splits,
            split_c, bp, int(bool(relu)) | (_lib.OCPPO_X6_MBITS_ROWS if mbits_rows else 0),
            None if mask is None else mask.data_ptr(),
            0 if mask is None else mask.stride(0), None if dbp is None else dbp.data_ptr(),
            None if mbits_out is None else mbits_out.data_ptr(),
            None if mbits_in is None else mbits_in.data_ptr(), t, -1 if mbig is None else int(mbig),
            None if b_planes is None else b_planes.data_ptr(), K, N * K,
            *((x6_sk_workspace(t, dev).data_ptr(), x6_sk_workspace(t, dev).numel())
              if stream_k else (None, 0)))
    # timer site name: the product's shape (bench.py's gemm_x6 roofline parses it); the closure
    # keeps the operand tensors alive for the timer's replays
    masked = mask is not None or mbits_in is not None
    name = f"gemm_x6_{M}x{N}x{K}s{splits}{'m' if masked else ''}"
    keep = (a, b, c, bias, mask, dbp, mbits_out, mbits_in, b_planes)
    _note_planes(b_planes, M, N, K)
    timed(name, lambda: call("ocppo_gemm_x6", _stream(dev), *args) or keep)
    return c


def linear_x6_ok(x, w) -> bool:
    """y = x W^T on gemm_x6: x [M, K], W [N, K] row-major f32, K % 32 == 0, a tile divides M x N."""
    return (_x6_operand_ok(x) and _x6_operand_ok(w) and x.shape[1] == w.shape[1]
            and x.shape[1] % 32 == 0 and x6_tile(x.shape[0], w.shape[0]) is not None)


def linear_x6(x, w, b=None, relu=False, out=None, mbits=False, planes=None):
    """act(x W^T + b) (torch._addmm_activation's order: sum, + bias, then ReLU). mbits=True
    (with relu) also returns the output's ReLU bitmask (tensor, tile) for dx_x6_relu; mbits="rows"
    the row-major one (int32 [M, N / 32] words, "rows") for frames_scatter_relu. planes: W's
    pre-split bf16 [3, N, K] (WeightPlanes; bitwise the same result)."""
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device) if out is None else out
    if not mbits:
        return gemm_x6(x, x.stride(0), 1, w, w.stride(0), 1, out, out.stride(0), M, N, K, bias=b,
                       relu=relu, b_planes=planes)
    if mbits == "rows":
        if not relu or N % 32:
            raise ValueError("linear_x6: the row-major bitmask needs relu and N % 32 == 0")
        bits = torch.empty((M, N // 32), dtype=torch.int32, device=x.device)
        gemm_x6(x, x.stride(0), 1, w, w.stride(0), 1, out, out.stride(0), M, N, K, bias=b,
                relu=relu, mbits_out=bits, mbits_rows=True, b_planes=planes)
        return out, (bits, "rows")
    t = x6_tile(M, N)
    bits = torch.empty(x6_mbits_words(M, N, t), dtype=torch.int64, device=x.device)
    gemm_x6(x, x.stride(0), 1, w, w.stride(0), 1, out, out.stride(0), M, N, K, bias=b,
            relu=relu, tile=t, mbits_out=bits, b_planes=planes)
    return out, (bits, t)


def x6_fwd_splits(M: int, N: int, K: int):
    """K splits for a forward product too small for one wave of 128 x 128 tiles (< 256 of them):
    the fewest splits reaching >= 512 workgroups (two per CU) with >= 256 k per split, on the
    128 x 128 tile; None when it does not apply. ([4096 x 512] from K = 2048, the decoder: 4
    splits, 56.8 vs 71.9 us for hipBLASLt's f32 GEMM + epilogue, tools/exp_decoder_fwd.py.)"""
    if M % 128 or N % 128 or K % 32:
        return None
    tiles = (M // 128) * (N // 128)
    if tiles >= 256 or tiles < 32:
        return None
    for S in (2, 4, 8, 16):
        if K % (32 * S) == 0 and K // S >= 256 and S * tiles >= 512:
            return S
    return None


def gemm_x6_gather(a, sam, sak, b, sbn, sbk, c, ldc, M, N, K, gidx, gw, gseg, mode, splits=1,
                   split_c=0, bias=None, relu=False, b_planes=None):
    """ocppo_gemm_x6_gather: gemm_x6 on the 128 x 128 tile with one operand's rows read through
    the row table gidx [rows, gw] (mode 1: A(m, k) = a[gidx[m, k // gseg] * sam + k % gseg];
    mode 2: B(n, k) = b[gidx[k, n // gseg] * sbk + n % gseg]). Same products as gemm_x6 on the
    materialised operand, bitwise."""
    dev = c.device
    f = torch.float32
    args = (a.data_ptr(), sam, sak, None if b_planes is not None else b.data_ptr(), sbn, sbk,
            c.data_ptr(), ldc, M, N, K, splits, split_c, _opt(bias, "bias", f, dev),
            int(bool(relu)), None if b_planes is None else b_planes.data_ptr(),
            _check(gidx, "gidx", torch.int32, dev), gw, gseg, int(mode))
    keep = (a, b, c, bias, b_planes, gidx)
    _note_planes(b_planes, M, N, K)
    timed(f"gemm_x6_{M}x{N}x{K}s{splits}",
          lambda: call("ocppo_gemm_x6_gather", _stream(dev), *args) or keep)
    return c


def linear_x6_split(x, w, b, relu, splits, out=None, planes=None, gather=None):
    """act(x W^T + b) as `splits` K-split gemm_x6 partials + ocppo_sum_splits_act (the partials
    added in split order in f64, then + bias, then ReLU). gather = (idx [M, W], E): x is the
    [C, E] row source and the product's input row m is the concatenation of x[idx[m, 0..W)]
    (frames_expand never materialised; one split per stack slot, splits == W)."""
    if gather is None:
        M, K = x.shape
    else:
        idx, E = gather
        M, K = idx.shape[0], idx.shape[1] * E
    N = w.shape[0]
    dev = x.device
    part = torch.empty((splits, M, N), dtype=torch.float32, device=dev)
    if gather is None:
        gemm_x6(x, x.stride(0), 1, w, w.stride(0), 1, part, N, M, N, K, splits=splits,
                split_c=M * N, tile=X6_AUTO, b_planes=planes)
    else:
        gemm_x6_gather(x, x.stride(0), 1, w, w.stride(0), 1, part, N, M, N, K, idx, idx.shape[1],
                       E, 1, splits=splits, split_c=M * N, b_planes=planes)
    out = torch.empty((M, N), dtype=torch.float32, device=dev) if out is None else out
    f = torch.float32
    args = (part.data_ptr(), splits, M, N, _opt(b, "bias", f, dev, N), int(bool(relu)),
            _check(out, "out", f, dev, M * N))
    keep = (part, out, b)
    timed(f"sum_splits_act_{splits}x{M}x{N}",
          lambda: call("ocppo_sum_splits_act", _stream(dev), *args) or keep)
    return out


def dx_x6_ok(g, w) -> bool:
    """dX = g W on gemm_x6: g [M, N] (N % 32 == 0), W [N, K]."""
    return (_x6_operand_ok(g) and _x6_operand_ok(w) and g.shape[1] == w.shape[0]
            and g.shape[1] % 32 == 0 and x6_tile(g.shape[0], w.shape[1]) is not None)


def dx_x6(g, w, out=None, planes=None, tile=None):
    """g W; planes: W^T's pre-split bf16 [3, K, N] (WeightPlanes); tile: None = x6_tile's."""
    M, N = g.shape
    K = w.shape[1]
    out = torch.empty((M, K), dtype=torch.float32, device=g.device) if out is None else out
    return gemm_x6(g, g.stride(0), 1, w, 1, w.stride(0), out, out.stride(0), M, K, N,
                   b_planes=planes, tile=tile)


def dx_x6_wgrad_ok(g, w, mask, x) -> bool:
    """dX = g W with the lower layer's backward in the epilogue (dx_x6_wgrad) applies."""
    M, N = g.shape
    K = w.shape[1]
    return (_x6_operand_ok(g) and w.is_cuda and w.dtype == torch.float32 and w.dim() == 2
            and w.stride(1) == 1 and w.stride(0) % 4 == 0 and w.data_ptr() % 16 == 0
            and w.shape[0] == N and N % 32 == 0 and M % 64 == 0 and K % 64 == 0
            and mask.is_cuda and mask.dtype == torch.float32 and mask.shape == (M, K)
            and mask.stride(1) == 1 and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
            and x.shape[0] == M and 1 <= x.shape[1] <= 16 and x.stride(1) == 1)


def dx_x6_wgrad(g, w, mask, x, dw, db, defer, tile=27):
    """The lower Linear+ReLU layer's (dw, db) from this layer's dX = g W without storing dX:
    gp = mask > 0 ? g W : 0, db = gp.sum(0), dw = gp^T x (ocppo_gemm_x6_wgrad; g [M, N], W [N, K],
    mask [M, K] the lower layer's ReLU output, x [M, K1] its input rows). The per-row-tile records
    are finished by the filled DeferredFinish `defer` (sum_splits_db(..., finish=) or run())."""
    M, N = g.shape
    K = w.shape[1]
    K1 = x.shape[1]
    dev = g.device
    bm = 64 if tile == 27 else 128
    kp = 4 if K1 <= 4 else 8 if K1 <= 8 else 12 if K1 <= 12 else 16
    nrec = (M // bm) * ((K + 255) // 256) * 256 * (kp + 1)
    rec = _persistent("dx_x6_wgrad", dev, (M, K, kp, tile),
                      lambda: torch.empty(nrec, dtype=torch.float32, device=dev))
    f = torch.float32
    args = (g.data_ptr(), g.stride(0), 1, w.data_ptr(), 1, w.stride(0), M, K, N,
            mask.data_ptr(), mask.stride(0), x.data_ptr(), x.stride(0), K1,
            _check(dw, "dw", f, dev, K * K1), _check(db, "db", f, dev, K), rec.data_ptr(),
            rec.numel(), int(tile), defer.ptr())
    keep = (g, w, mask, x, dw, db, rec)
    timed(f"gemm_x6_{M}x{K}x{N}s1w", lambda: call("ocppo_gemm_x6_wgrad", _stream(dev), *args)
          or keep)
    defer.pending = defer.filled = True


def dx_x6_relu(g, w, mask, mbits=None, planes=None):
    """gp = threshold_backward(g W, mask, 0) for the Linear+ReLU layer below whose output is
    `mask` [M, K], with that layer's bias-gradient partials: returns (gp, dbp [M / tile rows, K])
    (dbp summed in row-tile order by sum_splits_db). mbits = (bitmask, tile) from that layer's
    linear_x6(..., mbits=True): read instead of the f32 mask when this product has the same tile."""
    M, N = g.shape
    K = w.shape[1]
    t = x6_tile(M, K)
    gp = torch.empty((M, K), dtype=torch.float32, device=g.device)
    dbp = torch.empty((M // X6_TILES[t][0], K), dtype=torch.float32, device=g.device)
    if mbits is not None and mbits[1] == t:
        gemm_x6(g, g.stride(0), 1, w, 1, w.stride(0), gp, K, M, K, N, dbp=dbp, tile=t,
                mbits_in=mbits[0], b_planes=planes)
    else:
        gemm_x6(g, g.stride(0), 1, w, 1, w.stride(0), gp, K, M, K, N, mask=mask, dbp=dbp, tile=t,
                b_planes=planes)
    return gp, dbp


class WeightPlanes:
    """Pre-split bf16 planes of Linear weights for the update GEMMs' B operand (ocppo_gemm_x6 with
    b_planes): [3, N, K] of W for the forward, [3, K, N] of W^T for dX, written by ONE
    ocppo_split_planes launch per refresh (after every optimizer step: the trainer refreshes at
    the start of each minibatch). The parameters are views of a flat buffer at fixed addresses,
    so the job table is built once. Attaches w._ocppo_planes = {"fwd": ..., "dx": ...}."""

    def __init__(self, fwd=(), dx=()):
        jobs = []
        for ws, trans in ((fwd, 0), (dx, 1)):
            for w in ws:
                if w.dtype != torch.float32 or w.dim() != 2 or w.stride(1) != 1:
                    raise ValueError("WeightPlanes: row-major f32 weights")
                R, C = w.shape
                shape = (3, C, R) if trans else (3, R, C)
                if shape[2] % 8:
                    raise ValueError(f"WeightPlanes: plane rows of {shape[2]} elements")
                dst = torch.empty(shape, dtype=torch.bfloat16, device=w.device)
                d = getattr(w, "_ocppo_planes", None) or {}
                d["dx" if trans else "fwd"] = dst
                w._ocppo_planes = d
                jobs.append((w, trans, dst))
        self.jobs = jobs
        self.dev = jobs[0][0].device if jobs else None
        c = ctypes
        self.calls = []
        for i in range(0, len(jobs), 8):
            part = jobs[i:i + 8]
            n = len(part)
            arrs = ((c.c_void_p * n)(*[w.data_ptr() for w, _, _ in part]),
                    (c.c_int64 * n)(*[w.stride(0) for w, _, _ in part]),
                    (c.c_int64 * n)(*[w.shape[0] for w, _, _ in part]),
                    (c.c_int64 * n)(*[w.shape[1] for w, _, _ in part]),
                    (c.c_int * n)(*[t for _, t, _ in part]),
                    (c.c_void_p * n)(*[d.data_ptr() for _, _, d in part]))
            self.calls.append((n, arrs))

    def refresh(self):
        for n, arrs in self.calls:
            call("ocppo_split_planes", _stream(self.dev), n, *arrs)


def split_planes_ref(x):
    """The exact three-piece bf16 split of an f32 tensor in torch (round to nearest even at each
    step): the reference ocppo_split_planes / gemm_x6 are checked against (tests)."""
    x0 = x.to(torch.bfloat16)
    r1 = x - x0.float()
    x1 = r1.to(torch.bfloat16)
    x2 = (r1 - x1.float()).to(torch.bfloat16)
    return torch.stack([x0, x1, x2])


def dw_x6_ok(g, x, splits: int) -> bool:
    """dW = g^T x on gemm_x6 as `splits` partial products over the rows (in steps of 32)."""
    rows = g.shape[0]
    return (_x6_operand_ok(g) and _x6_operand_ok(x) and x.shape[0] == rows and splits >= 1
            and rows % 32 == 0 and rows // 32 >= splits
            and x6_tile(g.shape[1], x.shape[1], splits) is not None)


def dw_x6_parts(g, x, splits: int, part=None, tile=None):
    """part[s] = g[rows of split s]^T x[rows of split s] -> [splits, N, K], the rows split evenly
    in steps of 32 (combined by sum_splits / sum_splits_db in split order)."""
    rows, N = g.shape
    K = x.shape[1]
    part = (torch.empty((splits, N, K), dtype=torch.float32, device=g.device)
            if part is None else part)
    return gemm_x6(g, 1, g.stride(0), x, 1, x.stride(0), part, K, N, K, rows, splits=splits,
                   split_c=N * K, tile=tile)


def dw_x6_parts_gather(g, src, idx, splits: int, part=None):
    """dw_x6_parts with x never materialised: x[r] = concat(src[idx[r, 0..W)]) (src [C, E],
    idx [rows, W] int32; the 128 x 128 tile, rows / splits <= 1024) -> [splits, N, W * E]."""
    rows, N = g.shape
    W = idx.shape[1]
    E = src.shape[1]
    K = W * E
    part = (torch.empty((splits, N, K), dtype=torch.float32, device=g.device)
            if part is None else part)
    return gemm_x6_gather(g, 1, g.stride(0), src, 1, src.stride(0), part, K, N, K, rows, idx, W,
                          E, 2, splits=splits, split_c=N * K)


# ---------------------------------------------------------------------------------------------
# Frame-deduplicated PPObj minibatch encoder (ppo_atari_oc.py:566 through architectures/ppo.py:60-84)
# ---------------------------------------------------------------------------------------------
def _obs_TNWF(obs):
    if obs.dim() != 4:
        raise ValueError(f"obs must be [T+1, N, W, F], got {tuple(obs.shape)}")
    T1, N, W, F = obs.shape
    return T1 - 1, N, W, F


def frames_gather(obs, uniq, out=None):
    """x[c, :] = f32(frame with timeline id uniq[c]) of the rollout obs [T+1, N, W, F]
    (padding ids < 0 give zero rows). uniq [C] int32 -> x [C, F] f32."""
    T, N, W, F = _obs_TNWF(obs)
    dev = obs.device
    C = uniq.numel()
    if out is None:
        out = torch.empty((C, F), dtype=torch.float32, device=dev)
    call("ocppo_frames_gather", _stream(dev), _check(obs, "obs", None, dev),
         _DTYPE_CODE[obs.dtype], T, N, W, F, _check(uniq, "uniq", torch.int32, dev), C,
         _check(out, "out", torch.float32, dev, C * F))
    return out


def frames_gather_linear(obs, uniq, weight, bias=None, relu: bool = True, x_out=None,
                         h_out=None, index=None):
    """(x, h): frames_gather(obs, uniq) and act(x @ weight.T + bias) in one launch
    (ocppo_frames_gather_linear: the update's first encoder layer over the distinct frames).
    index = (pos_of, perm, dones[, out]): also frames_expand_index's row table in the same launch;
    returns (x, h, idx) then."""
    T, N, W, F = _obs_TNWF(obs)
    dev = obs.device
    C = uniq.numel()
    N1 = weight.shape[0]
    f = torch.float32
    if x_out is None:
        x_out = torch.empty((C, F), dtype=f, device=dev)
    if h_out is None:
        h_out = torch.empty((C, N1), dtype=f, device=dev)
    ix, idx = (None, None, 0, None, None), None
    if index is not None:
        pos_of, perm, dones = index[:3]
        M = perm.numel()
        idx = index[3] if len(index) > 3 else torch.empty((M, W), dtype=torch.int32, device=dev)
        ix = (_check(pos_of, "pos_of", torch.int32, dev, (T + W - 1) * N),
              _check(perm, "perm", torch.int64, dev), M,
              _check(dones, "dones", f, dev, (T + 1) * N), _check(idx, "idx", torch.int32, dev, M * W))
    call("ocppo_frames_gather_linear", _stream(dev), _check(obs, "obs", None, dev),
         _DTYPE_CODE[obs.dtype], T, N, W, F, _check(uniq, "uniq", torch.int32, dev), C,
         _check(weight, "weight", f, dev, N1 * F), _opt(bias, "bias", f, dev, N1), N1,
         int(bool(relu)), _check(x_out, "x_out", f, dev, C * F),
         _check(h_out, "h_out", f, dev, C * N1), *ix)
    return (x_out, h_out) if index is None else (x_out, h_out, idx)


def frames_expand(enc, pos_of, perm, dones, T: int, N: int, W: int, out=None):
    """h[i, k, :] = enc[pos_of[timeline id of slot k of sample perm[i]]] -> [M, W, E] f32.
    enc [C, E] f32, pos_of [(T+W-1)*N] int32, perm [M] int64, dones [T+1, N] f32."""
    C, E = enc.shape
    M = perm.numel()
    dev = enc.device
    if out is None:
        out = torch.empty((M, W, E), dtype=torch.float32, device=dev)
    call("ocppo_frames_expand", _stream(dev), _check(enc, "enc", torch.float32, dev), C, E,
         _check(pos_of, "pos_of", torch.int32, dev, (T + W - 1) * N),
         _check(perm, "perm", torch.int64, dev), M,
         _check(dones, "dones", torch.float32, dev, (T + 1) * N), T, N, W,
         _check(out, "out", torch.float32, dev, M * W * E))
    return out


def frames_expand_index(pos_of, perm, dones, T: int, N: int, W: int, out=None):
    """idx[i, k] = pos_of[timeline id of slot k of sample perm[i]] -> [M, W] int32: the source
    rows frames_expand copies, for the gathered decoder GEMMs (gemm_x6_gather)."""
    M = perm.numel()
    dev = perm.device
    if out is None:
        out = torch.empty((M, W), dtype=torch.int32, device=dev)
    call("ocppo_frames_expand_index", _stream(dev),
         _check(pos_of, "pos_of", torch.int32, dev, (T + W - 1) * N),
         _check(perm, "perm", torch.int64, dev), M,
         _check(dones, "dones", torch.float32, dev, (T + 1) * N), T, N, W,
         _check(out, "idx", torch.int32, dev, M * W))
    return out


def frames_scatter(dh, uniq, inv, mb: int, dones, T: int, N: int, W: int, out=None):
    """Backward of frames_expand: denc[c, :] = sum of dh[i, k, :] over the uses of frame uniq[c]
    by minibatch `mb` (inv [T*N] int32: position of each sample in the epoch permutation).
    dh [M, W, E] f32 -> denc [C, E] f32, deterministic."""
    M = dh.shape[0]
    E = dh.shape[-1]
    if dh.numel() != M * W * E:
        raise ValueError(f"dh must be [M, W, E] with W={W}, got {tuple(dh.shape)}")
    C = uniq.numel()
    dev = dh.device
    if out is None:
        out = torch.empty((C, E), dtype=torch.float32, device=dev)
    call("ocppo_frames_scatter", _stream(dev), _check(dh, "dh", torch.float32, dev), M, E,
         _check(uniq, "uniq", torch.int32, dev), C, _check(inv, "inv", torch.int32, dev, T * N),
         int(mb), _check(dones, "dones", torch.float32, dev, (T + 1) * N), T, N, W,
         _check(out, "out", torch.float32, dev, C * E))
    return out


def frames_scatter_relu(dh, uniq, inv, mb: int, dones, T: int, N: int, W: int, out=None,
                        gp=None, with_db: bool = True, mbits=None):
    """frames_scatter with the ReLU backward of the layer whose output `out` [C, E] encoded the
    frames: gp = out <= 0 ? 0 : denc (ocppo_frames_scatter_relu). mbits: that output's row-major
    ReLU bitmask (linear_x6(..., mbits="rows")), read instead of `out`. Returns (gp, (partials,
    chunks)): the bias-gradient chunk sums (16 frames per chunk; a per-shape persistent buffer,
    _persistent) for sum_splits_db, or (gp, None) without with_db."""
    M = dh.shape[0]
    E = dh.shape[-1]
    if dh.numel() != M * W * E:
        raise ValueError(f"dh must be [M, W, E] with W={W}, got {tuple(dh.shape)}")
    C = uniq.numel()
    dev = dh.device
    f = torch.float32
    if gp is None:
        gp = torch.empty((C, E), dtype=f, device=dev)
    part = None
    if with_db:
        def make():
            chunks = int(_lib.LIB.ocppo_frames_scatter_chunks(C))
            return torch.zeros((chunks, E), dtype=f, device=dev), chunks

        part = _persistent("frames_scatter_relu", dev, (C, E), make)
    call("ocppo_frames_scatter_relu", _stream(dev), _check(dh, "dh", f, dev), M, E,
         _check(uniq, "uniq", torch.int32, dev), C, _check(inv, "inv", torch.int32, dev, T * N),
         int(mb), _check(dones, "dones", f, dev, (T + 1) * N), T, N, W,
         _opt(out, "out", f, dev, C * E) if mbits is None else None,
         _opt(mbits, "mbits", torch.int32, dev, C * E // 32), _check(gp, "gp", f, dev, C * E),
         part[0].data_ptr() if part is not None else None)
    return gp, part


def frame_cache_shift(enc, fresh, done=None):
    """In-place shift of the rollout's frame-encoding cache (PPObj): enc [N, W, E] f32,
    fresh [N, E] f32 (row stride may exceed E), done [N] f32 or None:
    enc[n, w] = fresh[n] if done[n] or w == W-1 else enc[n, w+1]  (the frame stack's own rule,
    ppo_atari_oc.py:506 re-encoding all W frames every step is what this saves)."""
    dev = enc.device
    if enc.dim() != 3 or fresh.dim() != 2:
        raise ValueError(f"enc must be [N, W, E] and fresh [N, E], got {tuple(enc.shape)}, "
                         f"{tuple(fresh.shape)}")
    N, W, E = enc.shape
    if tuple(fresh.shape) != (N, E) or fresh.stride(1) != 1 or fresh.dtype != torch.float32 \
            or fresh.device != dev:
        raise ValueError("fresh must be an f32 [N, E] row-major view on enc's device")
    _stream(fresh.device)
    call("ocppo_frame_cache_shift", _stream(dev), _check(enc, "enc", torch.float32, dev),
         fresh.data_ptr(), fresh.stride(0) if N > 1 else E,
         _opt(done, "done", torch.float32, dev, N), N, W, E)
    return enc


def gather_rows(src, idx, out=None, scale255: bool = False):
    """out[i] = float32(src[idx[i]]) for src [B, ...] f32|bf16|u8 → out [M, ...] f32. A
    channels_last `out` [M, C, H, X] gets the rows in NHWC order (ocppo_gather_rows_cl), divided
    by 255 as NormalizeImg does when scale255."""
    dev = src.device
    M = idx.numel()
    R = src[0].numel() if src.shape[0] else 0
    if out is None:
        out = torch.empty((M,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
    if src.dtype not in _DTYPE_CODE:
        raise ValueError(f"unsupported src dtype {src.dtype}")
    if not out.is_contiguous():
        if not (out.dim() == 4 and out.is_contiguous(memory_format=torch.channels_last) and
                tuple(out.shape[1:]) == tuple(src.shape[1:]) and out.shape[0] == M and
                out.dtype == torch.float32 and out.device == dev):
            raise ValueError("out must be contiguous or a channels_last [M, C, H, X] f32 tensor")
        C = src.shape[1]
        call("ocppo_gather_rows_cl", _stream(dev), _check(src, "src", None, dev),
             _DTYPE_CODE[src.dtype], _check(idx, "idx", torch.int64, dev, M), M, C, R // C,
             out.data_ptr(), OCPPO_NET_SCALE_255 if scale255 else 0)
        return out
    if scale255:
        raise ValueError("scale255 needs a channels_last out (ocppo_gather_rows_cl)")
    call("ocppo_gather_rows", _stream(dev), _check(src, "src", None, dev), _DTYPE_CODE[src.dtype],
         _check(idx, "idx", torch.int64, dev, M), M, R,
         _check(out, "out", torch.float32, dev, M * R))
    return out


# ---------------------------------------------------------------------------------------------
# VecNormalize reward normalisation (ppo_atari_oc.py:414, SB3 2.0.0 semantics)
# ---------------------------------------------------------------------------------------------
def vecnorm_reward(reward, done, ret_state, rms_state, reward_out, gamma=0.99, epsilon=1e-8,
                   clip_reward=10.0):
    N = reward.numel()
    dev = reward.device
    f = torch.float32
    call("ocppo_vecnorm_reward", _stream(dev), _check(reward, "reward", f, dev),
         _check(done, "done", f, dev, N), N, float(gamma), float(epsilon), float(clip_reward),
         _check(ret_state, "ret_state", torch.float64, dev, N),
         _check(rms_state, "rms_state", torch.float64, dev, 3),
         _check(reward_out, "reward_out", f, dev, N))
    return reward_out


# ---------------------------------------------------------------------------------------------
# synthetic env (harness)
# ---------------------------------------------------------------------------------------------
def synth_env_step(seed: int, step_base, step_offset: int, actions, frame_out, reward_out,
                   done_out, ep_state=None):
    N = reward_out.numel()
    D = frame_out[0].numel()
    dev = frame_out.device
    pixel = frame_out.dtype == torch.uint8
    if not pixel and frame_out.dtype != torch.float32:
        raise ValueError("frame_out must be f32 (objects) or u8 (pixels)")
    call("ocppo_synth_env_step", _stream(dev), seed & 0xFFFFFFFFFFFFFFFF,
         _check(step_base, "step_base", torch.int64, dev, 1), int(step_offset),
         _opt(actions, "actions", torch.int64, dev, N), N, D, int(pixel),
         _check(frame_out, "frame_out", None, dev, N * D),
         _check(reward_out, "reward_out", torch.float32, dev, N),
         _check(done_out, "done_out", torch.float32, dev, N),
         _opt(ep_state, "ep_state", torch.float32, dev, N * 5))


def cartpole_step(seed: int, actions, state, counters, obs_out, reward_out=None, done_out=None,
                  ep_state=None):
    """One step (actions [N] i64) or, with actions None, a reset of N device CartPole-v1 envs
    (gymnasium 0.28.1 dynamics, TimeLimit 500, same-step auto-reset): state [N, 4] f64 and
    counters [N, 2] i64 in/out, obs_out [N, 4] f32, reward_out / done_out [N] f32."""
    N = obs_out.shape[0]
    dev = obs_out.device
    f = torch.float32
    call("ocppo_cartpole_step", _stream(dev), int(seed) & 0xFFFFFFFFFFFFFFFF,
         _opt(actions, "actions", torch.int64, dev, N), N,
         _check(state, "state", torch.float64, dev, 4 * N),
         _check(counters, "counters", torch.int64, dev, 2 * N),
         _check(obs_out, "obs_out", f, dev, 4 * N), _opt(reward_out, "reward_out", f, dev, N),
         _opt(done_out, "done_out", f, dev, N), _opt(ep_state, "ep_state", f, dev, 5 * N))


# ---------------------------------------------------------------------------------------------
# clip_grad_norm_ + Adam over flat buffers (ppo_atari_oc.py:608-610)
# ---------------------------------------------------------------------------------------------
OPT_STEP, OPT_TOTAL_NORM, OPT_CLIP_COEF = (_lib.OCPPO_OPT_STEP, _lib.OCPPO_OPT_TOTAL_NORM,
                                           _lib.OCPPO_OPT_CLIP_COEF)


FLAT_ALIGN = 64  # floats: every parameter / grad view in a flat buffer starts 256-B aligned


def flat_offsets(params):
    """Offsets of `params` in one flat f32 buffer, each rounded up to FLAT_ALIGN elements so the
    views keep the 16-B alignment the vectorised kernels (policy head, Adam) need; returns
    (offsets, total length)."""
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += -(-p.numel() // FLAT_ALIGN) * FLAT_ALIGN
    return offs, off


class FlatAdam:
    """Adam (torch.optim.Adam semantics, eps as given) + global-norm gradient clipping over ONE
    flat f32 parameter buffer. Construct it over the module's parameters: every parameter becomes
    a view of `self.params` and its `.grad` a view of `self.grads` (so the DP all-reduce is one
    call). `step()` is two HIP launches and is graph-capturable (step count, lr on device).

    A subclass is another update rule over the same buffers and the same step(): it names its
    entry, and with NO_PLANES (why it takes no plane jobs, the entry's arguments in their place)
    write_planes refuses."""

    ENTRY = "ocppo_clip_adam_step"
    NO_PLANES = None

    def __init__(self, params, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float = 0.0):
        params = [p for p in params if p.requires_grad]
        dev = params[0].device
        offs, n = flat_offsets(params)
        self.numel = n
        # zero padding between parameters is a fixed point of clip + Adam (g = m = v = p = 0)
        self.params = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(n, dtype=torch.float32, device=dev)
        for p, off in zip(params, offs):
            k = p.numel()
            if p.dtype != torch.float32:
                raise ValueError("FlatAdam needs f32 parameters")
            # same strides as the parameter (e.g. channels_last conv weights keep their layout)
            view = self.params[off:off + k].as_strided(p.shape, p.stride())
            view.copy_(p.detach())
            p.data = view
            p.grad = self.grads[off:off + k].as_strided(p.shape, p.stride())
            p._ocppo_direct_grad = True  # agents.py's autograd Functions write grads in place
        self.param_list = params
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.lr = torch.tensor(float(lr), dtype=torch.float32, device=dev)
        self.scalars = torch.zeros(_lib.OCPPO_OPT_NUM_SCALARS, dtype=torch.float32, device=dev)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.max_grad_norm = float(max_grad_norm)
        nb = _lib.LIB.ocppo_clip_adam_workspace_bytes(n)
        self.ws = torch.zeros(int(nb), dtype=torch.uint8, device=dev)
        # the entry's arguments after the workspace
        self._planes = ((0, None, None, None, None, None) if self.NO_PLANES is None
                        else self.NO_PLANES[1])

    def write_planes(self, jobs):
        """jobs [(weight, trans, planes)] (WeightPlanes.jobs): every step also writes each
        weight's new values as its three exact bf16 pieces ([3, N, K], or of W^T [3, K, N] with
        trans) into planes, so the next GEMMs need no split launch (ocppo_clip_adam_step's plane
        jobs, <= 8)."""
        jobs = list(jobs)
        if self.NO_PLANES is not None:
            if jobs:
                raise ValueError(self.NO_PLANES[0])
            return
        if len(jobs) > 8:
            raise ValueError("FlatAdam.write_planes: at most 8 weights")
        base = self.params.data_ptr()
        offs, rows, cols, trs, dsts = [], [], [], [], []
        for w, trans, d in jobs:
            off = (w.data_ptr() - base) // 4
            if (w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous()
                    or not 0 <= off < self.numel or d.dtype != torch.bfloat16
                    or d.numel() != 3 * w.numel() or not d.is_contiguous()):
                raise ValueError("FlatAdam.write_planes: a contiguous 2-D weight of this buffer "
                                 "and its bf16 [3, ...] planes")
            offs.append(off)
            rows.append(w.shape[0])
            cols.append(w.shape[1])
            trs.append(int(trans))
            dsts.append(d.data_ptr())
        c = ctypes
        n = len(jobs)
        self._planes = ((n, (c.c_int64 * n)(*offs), (c.c_int64 * n)(*rows),
                         (c.c_int64 * n)(*cols), (c.c_int * n)(*trs), (c.c_void_p * n)(*dsts))
                        if n else (0, None, None, None, None, None))
        self._plane_keep = [d for _, _, d in jobs]

    def zero_grad(self):
        self.grads.zero_()

    def step(self, grad_scale: float = 1.0):
        dev = self.params.device
        call(self.ENTRY, _stream(dev), self.params.data_ptr(), self.grads.data_ptr(),
             self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.numel,
             self.lr.data_ptr(), self.betas[0], self.betas[1], self.eps, float(grad_scale),
             self.max_grad_norm, self.scalars.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
             *self._planes)


# ---------------------------------------------------------------------------------------------
# DQN (config 5): HBM replay buffer, epsilon-greedy, fused TD target + MSE (dqn_atari_oc.py)
# ---------------------------------------------------------------------------------------------
class ReplayBuffer:
    """SB3 ReplayBuffer(optimize_memory_usage=True, handle_timeout_termination=False) in HBM
    (dqn_atari_oc.py:317-325): obs [size, E, D] in an exact compact dtype, next obs of slot i at
    slot i+1; device {pos, full} state so add/sample are graph-replayable."""

    def __init__(self, size: int, n_envs: int, obs_shape, device, obs_dtype=torch.uint8,
                 seed: int = 0):
        self.size, self.E = int(size), int(n_envs)
        self.obs_shape = tuple(obs_shape)
        self.D = 1
        for d in self.obs_shape:
            self.D *= d
        dev = torch.device(device)
        self.device = dev
        self.obs = torch.zeros((self.size, self.E) + self.obs_shape, dtype=obs_dtype, device=dev)
        self.actions = torch.zeros((self.size, self.E), dtype=torch.int64, device=dev)
        self.rewards = torch.zeros((self.size, self.E), dtype=torch.float32, device=dev)
        self.dones = torch.zeros((self.size, self.E), dtype=torch.float32, device=dev)
        self.state = torch.zeros(2, dtype=torch.int64, device=dev)  # pos, full
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ws = torch.zeros(int(_lib.LIB.ocppo_replay_workspace_bytes()), dtype=torch.uint8,
                              device=dev)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def add(self, obs, next_obs, actions, rewards, dones):
        dev = self.device
        f = torch.float32
        if obs.dtype not in _DTYPE_CODE or next_obs.dtype != obs.dtype:
            raise ValueError("obs/next_obs must both be f32, bf16 or u8")
        n = self.E * self.D
        call("ocppo_replay_add", _stream(dev), _check(obs, "obs", None, dev, n),
             _check(next_obs, "next_obs", None, dev, n), _DTYPE_CODE[obs.dtype],
             _check(actions, "actions", torch.int64, dev, self.E),
             _check(rewards, "rewards", f, dev, self.E), _check(dones, "dones", f, dev, self.E),
             self.E, self.D, self.state.data_ptr(), self.size, self.obs.data_ptr(),
             _DTYPE_CODE[self.obs.dtype], self.actions.data_ptr(), self.rewards.data_ptr(),
             self.dones.data_ptr(), self.ws.data_ptr())

    def sample(self, batch_size: int, out: dict | None = None, with_indices: bool = False):
        dev = self.device
        B = int(batch_size)
        if out is None:
            out = {"observations": torch.empty((B,) + self.obs_shape, device=dev),
                   "next_observations": torch.empty((B,) + self.obs_shape, device=dev),
                   "actions": torch.empty((B, 1), dtype=torch.int64, device=dev),
                   "rewards": torch.empty((B, 1), device=dev),
                   "dones": torch.empty((B, 1), device=dev)}
            if with_indices:
                out["indices"] = torch.empty((B, 2), dtype=torch.int64, device=dev)
        call("ocppo_replay_sample", _stream(dev), self.seed, self.counter.data_ptr(),
             self.state.data_ptr(), self.size, self.E, self.D, self.obs.data_ptr(),
             _DTYPE_CODE[self.obs.dtype], self.actions.data_ptr(), self.rewards.data_ptr(),
             self.dones.data_ptr(), B, out["observations"].data_ptr(),
             out["next_observations"].data_ptr(), out["actions"].data_ptr(),
             out["rewards"].data_ptr(), out["dones"].data_ptr(),
             out["indices"].data_ptr() if "indices" in out else None)
        return out


def epsilon_greedy(q, seed: int, step, start_e: float, end_e: float, duration: float,
                   actions_out=None, epsilon_out=None, step_offset: int = 0):
    E, A = q.shape
    dev = q.device
    if actions_out is None:
        actions_out = torch.empty(E, dtype=torch.int64, device=dev)
    call("ocppo_epsilon_greedy", _stream(dev), _check(q, "q", torch.float32, dev), E, A,
         int(seed) & 0xFFFFFFFFFFFFFFFF, _check(step, "step", torch.int64, dev, 1),
         int(step_offset), float(start_e),
         float(end_e), float(duration), _check(actions_out, "actions", torch.int64, dev, E),
         _opt(epsilon_out, "epsilon_out", torch.float32, dev, 1))
    return actions_out


def q_head_epsilon_greedy(hidden, wq, bq, seed: int, step, start_e: float, end_e: float,
                          duration: float, actions_out=None, epsilon_out=None,
                          step_offset: int = 0, q_out=None):
    """epsilon_greedy(hidden @ wq.T + bq, ...) in one launch (ocppo_q_head_epsilon_greedy)."""
    E, H = hidden.shape
    A = wq.shape[0]
    dev = hidden.device
    f = torch.float32
    if actions_out is None:
        actions_out = torch.empty(E, dtype=torch.int64, device=dev)
    call("ocppo_q_head_epsilon_greedy", _stream(dev), _check(hidden, "hidden", f, dev), E, H,
         _check(wq, "wq", f, dev, A * H), _check(bq, "bq", f, dev, A), A,
         int(seed) & 0xFFFFFFFFFFFFFFFF, _check(step, "step", torch.int64, dev, 1),
         int(step_offset), float(start_e), float(end_e), float(duration),
         _check(actions_out, "actions", torch.int64, dev, E),
         _opt(epsilon_out, "epsilon_out", f, dev, 1), _opt(q_out, "q_out", f, dev, E * A))
    return actions_out


def dqn_act_step_ok(hidden, wq, env, prev_obs, rb) -> bool:
    """dqn_act_step applies: <= 64 envs, the q_head_epsilon_greedy head shapes, an object-frame
    synthetic env and a replay in the stacks' dtype."""
    E, H = hidden.shape
    fr = getattr(env, "frame", None)
    return (getattr(env, "synthetic", False) and fr is not None and fr.dtype == torch.float32
            and fr.is_contiguous() and fr.shape[0] == E and 1 <= E <= 64
            and H % 256 == 0 and 256 <= H <= 1024 and 1 <= wq.shape[0] <= 8
            and hidden.is_contiguous() and wq.is_contiguous()
            and (hidden.data_ptr() | wq.data_ptr()) % 16 == 0
            and rb.obs.dtype == prev_obs.dtype and rb.E == E and prev_obs.is_contiguous()
            and rb.D == prev_obs[0].numel())


def dqn_act_step(hidden, wq, bq, seed: int, step, start_e: float, end_e: float, duration: float,
                 actions_out, epsilon_out, step_offset: int, env, env_step_offset: int, prev_obs,
                 obs_out, net_obs, done_out, reward_out, rb, vecnorm_state=None, gamma=0.99,
                 epsilon=1e-8, clip_reward=10.0, advance: int = 0):
    """q_head_epsilon_greedy + env.step + rollout_store(_vecnorm) + rb.add(prev_obs, obs_out,
    actions, reward_out, done_out) in one launch (ocppo_dqn_act_step; see dqn_act_step_ok);
    advance: then step += advance and env.advance(advance) in the same launch."""
    E, H = hidden.shape
    A = wq.shape[0]
    dev = hidden.device
    f = torch.float32
    W = obs_out.shape[1]
    D = env.frame.shape[1]
    if prev_obs.shape != obs_out.shape or prev_obs.dtype != obs_out.dtype or \
            obs_out[0, 0].numel() != D:
        raise ValueError("prev_obs / obs_out must be [E, W, D] stacks of one dtype")
    ret, rms = vecnorm_state if vecnorm_state is not None else (None, None)
    call("ocppo_dqn_act_step", _stream(dev), _check(hidden, "hidden", f, dev), E, H,
         _check(wq, "wq", f, dev, A * H), _check(bq, "bq", f, dev, A), A,
         int(seed) & 0xFFFFFFFFFFFFFFFF, _check(step, "step", torch.int64, dev, 1),
         int(step_offset), float(start_e), float(end_e), float(duration),
         _check(actions_out, "actions", torch.int64, dev, E),
         _opt(epsilon_out, "epsilon_out", f, dev, 1), env.seed & 0xFFFFFFFFFFFFFFFF,
         _check(env.step_base, "step_base", torch.int64, dev, 1), int(env_step_offset), D,
         _check(env.frame, "frame", f, dev, E * D), _check(env.reward, "reward", f, dev, E),
         _check(env.done, "done", f, dev, E), _opt(env.ep_state, "ep_state", f, dev, E * 5), W,
         _check(prev_obs, "prev_obs", None, dev, E * W * D),
         _check(obs_out, "obs_out", None, dev, E * W * D), _DTYPE_CODE[obs_out.dtype],
         _opt(net_obs, "net_obs", f, dev, E * W * D), _check(done_out, "done_out", f, dev, E),
         _check(reward_out, "reward_out", f, dev, E), int(vecnorm_state is not None),
         float(gamma), float(epsilon), float(clip_reward),
         _opt(ret, "ret_state", torch.float64, dev, E), _opt(rms, "rms_state", torch.float64, dev, 3),
         rb.state.data_ptr(), rb.size, rb.obs.data_ptr(), rb.actions.data_ptr(),
         rb.rewards.data_ptr(), rb.dones.data_ptr(), int(advance))
    return actions_out


def td_loss_fwd_bwd(q, q_next, actions, rewards, dones, gamma: float, dq=None, stats=None):
    """(stats [2] = {td_loss, mean q(s,a)}, dq [B, A] = d loss / d q)."""
    B, A = q.shape
    dev = q.device
    f = torch.float32
    if dq is None:
        dq = torch.empty_like(q)
    if stats is None:
        stats = torch.empty(2, dtype=f, device=dev)
    call("ocppo_td_loss_fwd_bwd", _stream(dev), _check(q, "q", f, dev),
         _check(q_next, "q_next", f, dev, B * A), _check(actions, "actions", torch.int64, dev, B),
         _check(rewards, "rewards", f, dev, B), _check(dones, "dones", f, dev, B), B, A,
         float(gamma), _check(dq, "dq", f, dev, B * A), _check(stats, "stats", f, dev, 2))
    return stats, dq


# ---------------------------------------------------------------------------------------------
# C51 (c51_atari_oc.py): expected-value epsilon-greedy, fused projection + cross-entropy loss
# ---------------------------------------------------------------------------------------------
C51_MAX_ATOMS, C51_MAX_ACTIONS = 128, 18


def _dist_shape(x, atoms, name: str, atoms_name: str = "atoms"):
    """(rows, A, N) of a [rows, A * N] head output (C51's logits, Rainbow's advantage) against the
    [N] support buffer, within the distributional kernels' limits."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{name}: expected a [rows, A * N] tensor")
    if not isinstance(atoms, torch.Tensor) or atoms.dim() != 1:
        raise ValueError(f"{atoms_name}: expected the [N] {atoms_name} buffer")
    rows, AN = x.shape
    N = atoms.shape[0]
    if not 2 <= N <= C51_MAX_ATOMS:
        raise ValueError(f"{atoms_name}: N={N}, need 2 <= N <= {C51_MAX_ATOMS}")
    if rows < 1 or AN % N or not 1 <= AN // N <= C51_MAX_ACTIONS:
        raise ValueError(f"{name}: shape {tuple(x.shape)} is not [rows >= 1, A * {N}] with "
                         f"1 <= A <= {C51_MAX_ACTIONS}")
    return rows, AN // N, N


def c51_epsilon_greedy(logits, atoms, seed: int, step, start_e: float, end_e: float,
                       duration: float, actions_out=None, epsilon_out=None, step_offset: int = 0,
                       q_out=None):
    """epsilon_greedy((softmax(logits.view(E, A, N), 2) * atoms).sum(2), ...) in one launch
    (QNetwork_C51.get_action's expected Q + c51_atari_oc.py:303-308)."""
    E, A, N = _dist_shape(logits, atoms, "logits")
    dev = logits.device
    f = torch.float32
    if actions_out is None:
        actions_out = torch.empty(E, dtype=torch.int64, device=dev)
    call("ocppo_c51_epsilon_greedy", _stream(dev), _check(logits, "logits", f, dev),
         _check(atoms, "atoms", f, dev), E, A, N, int(seed) & 0xFFFFFFFFFFFFFFFF,
         _check(step, "step", torch.int64, dev, 1), int(step_offset), float(start_e),
         float(end_e), float(duration), _check(actions_out, "actions", torch.int64, dev, E),
         _opt(epsilon_out, "epsilon_out", f, dev, 1), _opt(q_out, "q_out", f, dev, E * A))
    return actions_out


def c51_loss_fwd_bwd(logits, logits_next, atoms, actions, rewards, dones, gamma: float,
                     v_min: float, v_max: float, dlogits=None, stats=None, target_pmfs=None,
                     next_action=None):
    """c51_atari_oc.py:339-359 and its backward in one launch: (stats [2] = {loss, mean expected
    Q of the taken actions}, dlogits [B, A * N] = d loss / d logits). target_pmfs [B, N] f32 and
    next_action [B] i64, when given, receive the projected target distribution and the target
    net's greedy next action."""
    B, A, N = _dist_shape(logits, atoms, "logits")
    dev = logits.device
    f = torch.float32
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    if stats is None:
        stats = torch.empty(2, dtype=f, device=dev)
    call("ocppo_c51_loss_fwd_bwd", _stream(dev), _check(logits, "logits", f, dev),
         _check(logits_next, "logits_next", f, dev, B * A * N), _check(atoms, "atoms", f, dev),
         _check(actions, "actions", torch.int64, dev, B), _check(rewards, "rewards", f, dev, B),
         _check(dones, "dones", f, dev, B), B, A, N, float(gamma), float(v_min), float(v_max),
         _check(dlogits, "dlogits", f, dev, B * A * N), _check(stats, "stats", f, dev, 2),
         _opt(target_pmfs, "target_pmfs", f, dev, B * N),
         _opt(next_action, "next_action", torch.int64, dev, B))
    return stats, dlogits


# ---------------------------------------------------------------------------------------------
# Rainbow (rainbow_atari_oc.py): device prioritized n-step replay, fused double-Q projection +
# weighted cross-entropy loss through the dueling heads, greedy acting
# ---------------------------------------------------------------------------------------------
PER_MAX_NSTEP, PER_MAX_BATCH = 8, 1024


class PrioritizedReplay:
    """PrioritizedReplayBuffer + SumSegmentTree (rainbow_atari_oc.py:338-499) in HBM for one env:
    obs / next_obs rows [capacity, D] in an exact compact dtype, the f32 sum tree in the
    reference's layout, the n-step ring, and a device state block {pos, size, max_priority, ring
    fill, ring head}, so add / sample / update_priorities replay from a hipGraph. beta follows
    the device step counter (`step` + step_offset) when sample() is given one."""

    def __init__(self, capacity: int, obs_shape, device, n_step: int, gamma: float,
                 alpha: float = 0.6, beta: float = 0.4, eps: float = 1e-6,
                 total_timesteps: float = 1.0, obs_dtype=torch.uint8, seed: int = 0,
                 num_envs: int = 1):
        if num_envs != 1:
            raise ValueError("PrioritizedReplay: vectorized envs are not supported (num_envs == 1)")
        if not 1 <= int(n_step) <= PER_MAX_NSTEP:
            raise ValueError(f"PrioritizedReplay: n_step={n_step}, need 1 <= n_step <= {PER_MAX_NSTEP}")
        if int(capacity) < 2:
            raise ValueError("PrioritizedReplay: capacity must be >= 2")
        if obs_dtype not in _DTYPE_CODE:
            raise ValueError("PrioritizedReplay: obs_dtype must be f32, bf16 or u8")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"PrioritizedReplay: HIP kernels need a GPU, got device {dev}")
        self.capacity, self.n_step = int(capacity), int(n_step)
        self.obs_shape = tuple(obs_shape)
        self.D = 1
        for d in self.obs_shape:
            self.D *= d
        self.device = dev
        self.gamma, self.alpha, self.beta, self.eps = float(gamma), float(alpha), float(beta), float(eps)
        self.total_timesteps = float(total_timesteps)
        # the n_step powers gamma ** i in Python's arithmetic (:428)
        self.gamma_pows = (ctypes.c_double * self.n_step)(*[self.gamma ** i for i in range(self.n_step)])
        C, n, f, i64 = self.capacity, self.n_step, torch.float32, torch.int64
        self.obs = torch.zeros((C,) + self.obs_shape, dtype=obs_dtype, device=dev)
        self.next_obs = torch.zeros((C,) + self.obs_shape, dtype=obs_dtype, device=dev)
        self.actions = torch.zeros(C, dtype=i64, device=dev)
        self.rewards = torch.zeros(C, dtype=f, device=dev)
        self.dones = torch.zeros(C, dtype=f, device=dev)
        self.tree = torch.zeros(2 * C - 1, dtype=f, device=dev)
        self.state = torch.zeros(8, dtype=i64, device=dev)
        self.state.view(f)[4] = 1.0  # max_priority (:414)
        self.ring_obs = torch.zeros((n,) + self.obs_shape, dtype=obs_dtype, device=dev)
        self.ring_next_obs = torch.zeros((n,) + self.obs_shape, dtype=obs_dtype, device=dev)
        self.ring_actions = torch.zeros(n, dtype=i64, device=dev)
        self.ring_rewards = torch.zeros(n, dtype=f, device=dev)
        self.ring_dones = torch.zeros(n, dtype=f, device=dev)
        self.counter = torch.zeros(1, dtype=i64, device=dev)
        self.beta_dev = torch.full((1,), self.beta, dtype=f, device=dev)
        self.ws = torch.zeros(int(_lib.LIB.ocppo_per_workspace_bytes()), dtype=torch.uint8,
                              device=dev)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    @property
    def max_priority(self) -> float:
        return float(self.state.view(torch.float32)[4])

    def add(self, obs, next_obs, actions, rewards, dones):
        """rb.add(obs, actions, rewards, real_next_obs, terminations) (:642) of the one env."""
        dev, f = self.device, torch.float32
        if not isinstance(obs, torch.Tensor) or obs.dtype not in _DTYPE_CODE or \
                next_obs.dtype != obs.dtype:
            raise ValueError("obs/next_obs must both be f32, bf16 or u8 tensors")
        call("ocppo_per_add", _stream(dev), _check(obs, "obs", None, dev, self.D),
             _check(next_obs, "next_obs", None, dev, self.D), _DTYPE_CODE[obs.dtype],
             _check(actions, "actions", torch.int64, dev, 1), _check(rewards, "rewards", f, dev, 1),
             _check(dones, "dones", f, dev, 1), self.D, self.n_step, self.gamma_pows, self.alpha,
             self.state.data_ptr(), self.capacity, self.obs.data_ptr(), self.next_obs.data_ptr(),
             _DTYPE_CODE[self.obs.dtype], self.actions.data_ptr(), self.rewards.data_ptr(),
             self.dones.data_ptr(), self.tree.data_ptr(), self.ring_obs.data_ptr(),
             self.ring_next_obs.data_ptr(), self.ring_actions.data_ptr(),
             self.ring_rewards.data_ptr(), self.ring_dones.data_ptr(), self.ws.data_ptr())

    def new_batch(self, batch_size: int, probs: bool = False, upperbounds: bool = False) -> dict:
        B, dev, f = int(batch_size), self.device, torch.float32
        out = {"observations": torch.zeros((B,) + self.obs_shape, device=dev),
               "next_observations": torch.zeros((B,) + self.obs_shape, device=dev),
               "actions": torch.zeros((B, 1), dtype=torch.int64, device=dev),
               "rewards": torch.zeros((B, 1), device=dev), "dones": torch.zeros((B, 1), device=dev),
               "indices": torch.zeros(B, dtype=torch.int64, device=dev),
               "weights": torch.zeros((B, 1), dtype=f, device=dev)}
        if probs:
            out["probs"] = torch.zeros(B, dtype=f, device=dev)
        if upperbounds:
            out["upperbounds"] = torch.zeros(B, dtype=torch.float64, device=dev)
        return out

    def sample(self, batch_size: int, out: dict | None = None, step=None, step_offset: int = 0,
               upperbounds_in=None):
        """(:462-490) `out` (new_batch) receives observations, next_observations, actions,
        rewards, dones, indices, weights and, where present, probs / upperbounds. beta =
        min(1, self.beta + (step + step_offset) * (1 - self.beta) / total_timesteps), or
        self.beta without `step`; upperbounds_in [B] f64 replaces the draws."""
        dev, f = self.device, torch.float32
        B = int(batch_size)
        if not 1 <= B <= PER_MAX_BATCH:
            raise ValueError(f"batch_size={B}: need 1 <= batch_size <= {PER_MAX_BATCH}")
        if out is None:
            out = self.new_batch(B)
        n = B * self.D
        call("ocppo_per_sample", _stream(dev), self.seed, self.counter.data_ptr(),
             self.state.data_ptr(), _opt(step, "step", torch.int64, dev, 1), int(step_offset),
             self.beta, self.total_timesteps, self.capacity, self.D, self.obs.data_ptr(),
             self.next_obs.data_ptr(), _DTYPE_CODE[self.obs.dtype], self.actions.data_ptr(),
             self.rewards.data_ptr(), self.dones.data_ptr(), self.tree.data_ptr(), B,
             _opt(upperbounds_in, "upperbounds_in", torch.float64, dev, B),
             _check(out["observations"], "observations", f, dev, n),
             _check(out["next_observations"], "next_observations", f, dev, n),
             _check(out["actions"], "actions", torch.int64, dev, B),
             _check(out["rewards"], "rewards", f, dev, B), _check(out["dones"], "dones", f, dev, B),
             _check(out["indices"], "indices", torch.int64, dev, B),
             _check(out["weights"], "weights", f, dev, B),
             _opt(out.get("probs"), "probs", f, dev, B),
             _opt(out.get("upperbounds"), "upperbounds", torch.float64, dev, B),
             self.beta_dev.data_ptr())
        return out

    def update_priorities(self, indices, loss_per_sample):
        """(:492-499) straight from the loss kernel's device output."""
        dev = self.device
        B = indices.numel() if isinstance(indices, torch.Tensor) else 0
        if not 1 <= B <= PER_MAX_BATCH:
            raise ValueError(f"indices: need 1 <= B <= {PER_MAX_BATCH} elements")
        call("ocppo_per_update_priorities", _stream(dev),
             _check(indices, "indices", torch.int64, dev, B),
             _check(loss_per_sample, "loss_per_sample", torch.float32, dev, B), B, self.eps,
             self.alpha, self.state.data_ptr(), self.capacity, self.tree.data_ptr())


def _rainbow_shape(value, advantage, support, name: str):
    """(rows, A, N) of value [rows, N] / advantage [rows, A * N] against the [N] support."""
    rows, A, N = _dist_shape(advantage, support, f"{name}: advantage", "support")
    if not isinstance(value, torch.Tensor) or tuple(value.shape) != (rows, N):
        raise ValueError(f"{name}: value must be [{rows}, {N}]")
    return rows, A, N


def rainbow_greedy(value, advantage, support, actions_out=None, q_out=None):
    """argmax_a (softmax(value + advantage - mean_a advantage, atoms) * support).sum(atoms) in one
    launch (rainbow_atari_oc.py:617-620), first maximum."""
    E, A, N = _rainbow_shape(value, advantage, support, "rainbow_greedy")
    dev, f = value.device, torch.float32
    if actions_out is None:
        actions_out = torch.empty(E, dtype=torch.int64, device=dev)
    call("ocppo_rainbow_greedy", _stream(dev), _check(value, "value", f, dev),
         _check(advantage, "advantage", f, dev), _check(support, "support", f, dev), E, A, N,
         _check(actions_out, "actions", torch.int64, dev, E), _opt(q_out, "q_out", f, dev, E * A))
    return actions_out


def rainbow_loss_fwd_bwd(value, advantage, value_next_online, advantage_next_online,
                         value_next_target, advantage_next_target, support, actions, rewards,
                         dones, weights, gamma_n: float, v_min: float, v_max: float, dvalue=None,
                         dadvantage=None, loss_per_sample=None, stats=None, target_pmfs=None,
                         best_actions=None):
    """rainbow_atari_oc.py:655-701 and its backward in one launch, on the raw head outputs of the
    three forwards. Returns (stats [2] = {loss, mean expected Q of the taken actions},
    loss_per_sample [B], dvalue [B, N], dadvantage [B, A * N])."""
    B, A, N = _rainbow_shape(value, advantage, support, "rainbow_loss_fwd_bwd")
    dev, f = value.device, torch.float32
    if dvalue is None:
        dvalue = torch.empty_like(value)
    if dadvantage is None:
        dadvantage = torch.empty_like(advantage)
    if loss_per_sample is None:
        loss_per_sample = torch.empty(B, dtype=f, device=dev)
    if stats is None:
        stats = torch.empty(2, dtype=f, device=dev)
    call("ocppo_rainbow_loss_fwd_bwd", _stream(dev), _check(value, "value", f, dev),
         _check(advantage, "advantage", f, dev),
         _check(value_next_online, "value_next_online", f, dev, B * N),
         _check(advantage_next_online, "advantage_next_online", f, dev, B * A * N),
         _check(value_next_target, "value_next_target", f, dev, B * N),
         _check(advantage_next_target, "advantage_next_target", f, dev, B * A * N),
         _check(support, "support", f, dev), _check(actions, "actions", torch.int64, dev, B),
         _check(rewards, "rewards", f, dev, B), _check(dones, "dones", f, dev, B),
         _check(weights, "weights", f, dev, B), B, A, N, float(gamma_n), float(v_min),
         float(v_max), _check(dvalue, "dvalue", f, dev, B * N),
         _check(dadvantage, "dadvantage", f, dev, B * A * N),
         _check(loss_per_sample, "loss_per_sample", f, dev, B), _check(stats, "stats", f, dev, 2),
         _opt(target_pmfs, "target_pmfs", f, dev, B * N),
         _opt(best_actions, "best_actions", torch.int64, dev, B))
    return stats, loss_per_sample, dvalue, dadvantage


# ---------------------------------------------------------------------------------------------
# transformer encoder blocks (ppo_atari_oc_transformer.py:215-277: torch's TransformerEncoderLayer)
# ---------------------------------------------------------------------------------------------
MHA_MAX_S, MHA_MAX_E, MHA_HEAD_DIMS = 64, 512, (8, 16, 32, 64)


def mha_shape_ok(S: int, E: int, heads: int) -> bool:
    """The contract of ocppo_mha_fwd / ocppo_mha_bwd."""
    return (1 <= S <= MHA_MAX_S and 1 <= E <= MHA_MAX_E and heads >= 1 and E % heads == 0 and
            E // heads in MHA_HEAD_DIMS)


def _mha_shape(qkv, key_valid, heads: int, who: str):
    if qkv.dim() != 3 or qkv.shape[2] % 3:
        raise ValueError(f"{who}: qkv must be [B, S, 3E], got {tuple(qkv.shape)}")
    B, S, E3 = qkv.shape
    E = E3 // 3
    if B < 1 or not mha_shape_ok(S, E, heads):
        raise ValueError(f"{who}: unsupported B={B} S={S} E={E} heads={heads} (mha_shape_ok)")
    kv = _opt(key_valid, "key_valid", torch.uint8, qkv.device, B * S)
    return B, S, E, kv


def mha_fwd(qkv, key_valid, heads: int, out=None, lse=None):
    """Masked multi-head self-attention (nn.MultiheadAttention's math): qkv [B, S, 3E] f32 (the
    in-proj output, q | k | v), key_valid [B, S] u8 or None -> (out [B, S, E], lse [B, heads, S])."""
    B, S, E, kv = _mha_shape(qkv, key_valid, heads, "mha_fwd")
    dev, f = qkv.device, torch.float32
    out = torch.empty((B, S, E), dtype=f, device=dev) if out is None else out
    lse = torch.empty((B, heads, S), dtype=f, device=dev) if lse is None else lse
    call("ocppo_mha_fwd", _stream(dev), _check(qkv, "qkv", f, dev), kv, B, S, E, heads,
         _check(out, "out", f, dev, B * S * E), _check(lse, "lse", f, dev, B * heads * S))
    return out, lse


def mha_bwd(qkv, key_valid, out, lse, dout, heads: int, dqkv=None):
    """d qkv [B, S, 3E] of mha_fwd (every element written; excluded keys' dK / dV exactly 0)."""
    B, S, E, kv = _mha_shape(qkv, key_valid, heads, "mha_bwd")
    dev, f = qkv.device, torch.float32
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    call("ocppo_mha_bwd", _stream(dev), _check(qkv, "qkv", f, dev), kv,
         _check(out, "out", f, dev, B * S * E), _check(lse, "lse", f, dev, B * heads * S),
         _check(dout, "dout", f, dev, B * S * E), B, S, E, heads,
         _check(dqkv, "dqkv", f, dev, B * S * 3 * E))
    return dqkv


class _MHA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, key_valid, heads: int):
        qkv = qkv.detach().contiguous()
        out, lse = mha_fwd(qkv, key_valid, heads)
        ctx.save_for_backward(qkv, key_valid, out, lse)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, key_valid, out, lse = ctx.saved_tensors
        return mha_bwd(qkv, key_valid, out, lse, g.contiguous(), ctx.heads), None, None


# ---- counter-based dropout (include/ocppo.h, ABI 33) ---------------------------
# The dropout contract of the attention kernels: every head dim of MHA_HEAD_DIMS (the dh = 64
# backward instantiation compiles to 256 VGPRs without scratch, as the p = 0 one does).
MHA_DROPOUT_HEAD_DIMS = MHA_HEAD_DIMS
DROPOUT_SITES = 256


def mha_dropout_shape_ok(S: int, E: int, heads: int) -> bool:
    """The contract of ocppo_mha_dropout_fwd / ocppo_mha_dropout_bwd."""
    return mha_shape_ok(S, E, heads) and E // heads in MHA_DROPOUT_HEAD_DIMS


def dropout_consts(p: float):
    """(thr, scale) of a drop probability: keep iff word >= thr = min(int(p * 2^32), 2^32 - 1);
    scale = 1 / (1 - p) in double (the entry points take it as f32)."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout: p = {p} not in [0, 1)")
    return min(int(p * 2 ** 32), 2 ** 32 - 1), 1.0 / (1.0 - p)


def _drop_args(rng, site: int, p: float, dev, who: str):
    """(rng pointer, site, thr, scale) of a launch that draws a mask."""
    thr, scale = dropout_consts(p)
    if isinstance(site, bool) or not isinstance(site, int) or not 0 <= site < DROPOUT_SITES:
        raise ValueError(f"{who}: site {site!r} not an integer in [0, {DROPOUT_SITES})")
    if rng is None:
        raise ValueError(f"{who}: p = {p} > 0 needs the generator state rng (i64 [seed, offset])")
    return _check(rng, "rng", torch.int64, dev, 2), site, thr, scale


def philox_state(seed: int, device, offset: int = 0):
    """A dropout generator state: device i64 [seed, offset]."""
    return torch.tensor([int(seed), int(offset)], dtype=torch.int64, device=device)


def philox_advance(rng):
    """rng[1] += 1 on the device (one thread; graph-capturable)."""
    dev = rng.device
    call("ocppo_philox_advance", _stream(dev), _check(rng, "rng", torch.int64, dev, 2))
    return rng


def dropout_fwd(x, rng, site: int, p: float, out=None):
    """y = keep ? x / (1 - p) : 0 with the mask of (rng, site) over x's flat index; out of place.
    The backward is the same call on dy."""
    dev, f = x.device, torch.float32
    rp, site, thr, scale = _drop_args(rng, site, p, dev, "dropout")
    xp = _check(x, "x", f, dev)
    out = torch.empty_like(x) if out is None else out
    call("ocppo_dropout", _stream(dev), xp, rp, site, thr, scale, x.numel(),
         _check(out, "out", f, dev, x.numel()))
    return out


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rng, site: int, p: float):
        ctx.save_for_backward(rng)
        ctx.site, ctx.p = site, p
        return dropout_fwd(x.detach().contiguous(), rng, site, p)

    @staticmethod
    def backward(ctx, g):
        (rng,) = ctx.saved_tensors
        return dropout_fwd(g.contiguous(), rng, ctx.site, ctx.p), None, None, None


def dropout(x, rng, site: int, p: float):
    """Differentiable counter-based dropout; the backward regenerates the mask from the SAME rng
    tensor (give every site of one forward a snapshot of the live state). p == 0 launches nothing
    and returns x."""
    dropout_consts(p)
    if p == 0:
        return x
    _drop_args(rng, site, p, x.device, "dropout")
    return _Dropout.apply(x, rng, site, float(p))


def _mha_dropout_shape(qkv, key_valid, heads: int, who: str):
    B, S, E, kv = _mha_shape(qkv, key_valid, heads, who)
    if not mha_dropout_shape_ok(S, E, heads):
        raise ValueError(f"{who}: unsupported S={S} E={E} heads={heads} (mha_dropout_shape_ok)")
    return B, S, E, kv


def mha_dropout_fwd(qkv, key_valid, heads: int, rng, site: int, p: float, out=None, lse=None):
    """mha_fwd with dropout p on the attention probabilities (mask of (rng, site); lse unchanged)."""
    B, S, E, kv = _mha_dropout_shape(qkv, key_valid, heads, "mha_dropout_fwd")
    dev, f = qkv.device, torch.float32
    rp, site, thr, scale = _drop_args(rng, site, p, dev, "mha_dropout_fwd")
    out = torch.empty((B, S, E), dtype=f, device=dev) if out is None else out
    lse = torch.empty((B, heads, S), dtype=f, device=dev) if lse is None else lse
    call("ocppo_mha_dropout_fwd", _stream(dev), _check(qkv, "qkv", f, dev), kv, rp, site, thr,
         scale, B, S, E, heads, _check(out, "out", f, dev, B * S * E),
         _check(lse, "lse", f, dev, B * heads * S))
    return out, lse


def mha_dropout_bwd(qkv, key_valid, out, lse, dout, heads: int, rng, site: int, p: float,
                    dqkv=None):
    """d qkv of mha_dropout_fwd at the same (rng, site, p)."""
    B, S, E, kv = _mha_dropout_shape(qkv, key_valid, heads, "mha_dropout_bwd")
    dev, f = qkv.device, torch.float32
    rp, site, thr, scale = _drop_args(rng, site, p, dev, "mha_dropout_bwd")
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    call("ocppo_mha_dropout_bwd", _stream(dev), _check(qkv, "qkv", f, dev), kv,
         _check(out, "out", f, dev, B * S * E), _check(lse, "lse", f, dev, B * heads * S),
         _check(dout, "dout", f, dev, B * S * E), rp, site, thr, scale, B, S, E, heads,
         _check(dqkv, "dqkv", f, dev, B * S * 3 * E))
    return dqkv


class _MHADropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, key_valid, heads: int, rng, site: int, p: float):
        qkv = qkv.detach().contiguous()
        out, lse = mha_dropout_fwd(qkv, key_valid, heads, rng, site, p)
        ctx.save_for_backward(qkv, key_valid, out, lse, rng)
        ctx.heads, ctx.site, ctx.p = heads, site, p
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, key_valid, out, lse, rng = ctx.saved_tensors
        return (mha_dropout_bwd(qkv, key_valid, out, lse, g.contiguous(), ctx.heads, rng,
                                ctx.site, ctx.p), None, None, None, None, None)


def mha(qkv, key_valid, heads: int, rng=None, site: int = 0, p: float = 0.0):
    """Differentiable mha_fwd: [B, S, 3E] -> [B, S, E] (the heads concatenated, for out_proj).
    p > 0: dropout on the attention probabilities with the mask of (rng, site); the backward
    reads the same rng tensor. p == 0 is the path without dropout, whatever rng is."""
    dropout_consts(p)
    if p == 0:
        return _MHA.apply(qkv, key_valid, heads)
    return _MHADropout.apply(qkv, key_valid, heads, rng, site, float(p))


# The two LayerNorms (add_layernorm_* here, ln_relu_* with the PQN kernels below) are one kernel
# skeleton (csrc/ocppo_layernorm.h) behind two pairs of entries; so are their wrappers.
def _ln_shape(x, res, weight, bias, max_e: int, who: str):
    """(rows, E) of a LayerNorm over x's last dim."""
    E = x.shape[-1] if x.dim() else 0
    if (not 1 <= E <= max_e or weight.numel() != E or (bias is not None and bias.numel() != E)
            or (res is not None and res.shape != x.shape)):
        shapes = [f"{n} {tuple(t.shape)}" for n, t in (("x", x), ("res", res), ("weight", weight),
                                                       ("bias", bias)) if t is not None]
        raise ValueError(f"{who}: {', '.join(shapes)} (one weight and bias per element of the "
                         f"last dim, 1 <= last dim <= {max_e}, res shaped as x)")
    return x.numel() // E, E


def _ln_fwd(entry: str, x, res, weight, bias, eps: float, max_e: int, flags=()):
    """`entry`'s launch -> (y, mean [R], rstd [R]); res (or None) and flags as the entry takes
    them."""
    R, E = _ln_shape(x, res, weight, bias, max_e, entry)
    dev, f = x.device, torch.float32
    rows = [_check(t, n, f, dev) for n, t in (("x", x), ("res", res)) if t is not None]
    y = torch.empty_like(x)
    mean = torch.empty(R, dtype=f, device=dev)
    rstd = torch.empty(R, dtype=f, device=dev)
    call(entry, _stream(dev), *rows, _check(weight, "weight", f, dev, E),
         _check(bias, "bias", f, dev, E), R, E, float(eps), *flags, y.data_ptr(), mean.data_ptr(),
         rstd.data_ptr())
    return y, mean, rstd


def _ln_bwd(entry: str, workspace, dy, x, weight, mean, rstd, max_e: int, res=None, y=None,
            flags=()):
    """`entry`'s two launches (rows + per-workgroup partials, then their ordered sum) ->
    (dx, dweight, dbias). res or y: the entry's third row input (y may be None); workspace(bytes,
    device): the partials' buffer, fully written before it is read."""
    R, E = _ln_shape(x, res, weight, None, max_e, entry)
    dev, f = x.device, torch.float32
    dx = torch.empty_like(x)
    dw = torch.empty(E, dtype=f, device=dev)
    db = torch.empty(E, dtype=f, device=dev)
    nb = int(getattr(_lib.LIB, entry.replace("_bwd", "_workspace_bytes"))(R, E))
    ws = workspace(nb, dev)
    third = ("res", res) if res is not None else ("y", y)
    call(entry, _stream(dev), _check(dy, "dy", f, dev, R * E), _check(x, "x", f, dev),
         _opt(third[1], third[0], f, dev, R * E), _check(weight, "weight", f, dev, E),
         _check(mean, "mean", f, dev, R), _check(rstd, "rstd", f, dev, R), R, E, *flags,
         dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb)
    return dx, dw, db


def add_layernorm_fwd(x, res, weight, bias, eps: float):
    """LayerNorm(x + res) * weight + bias over the last dim -> (y, mean [R], rstd [R])."""
    return _ln_fwd("ocppo_add_layernorm_fwd", x, res, weight, bias, eps, MHA_MAX_E)


def add_layernorm_bwd(dy, x, res, weight, mean, rstd):
    """(dx, dweight, dbias) of add_layernorm_fwd; x + res is recomputed from the two inputs, dx
    is the gradient of both."""
    return _ln_bwd("ocppo_add_layernorm_bwd",
                   lambda nb, dev: torch.empty(nb // 4, dtype=torch.float32, device=dev),
                   dy, x, weight, mean, rstd, MHA_MAX_E, res=res)


class _AddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, weight, bias, eps: float):
        x, res = x.detach().contiguous(), res.detach().contiguous()
        w = weight.detach()
        y, mean, rstd = add_layernorm_fwd(x, res, w, bias.detach(), eps)
        ctx.save_for_backward(x, res, w, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, g):
        x, res, w, mean, rstd = ctx.saved_tensors
        dx, dw, db = add_layernorm_bwd(g.contiguous(), x, res, w, mean, rstd)
        return dx, dx, dw, db, None


def add_layernorm(x, res, weight, bias, eps: float = 1e-5):
    """Differentiable LayerNorm(x + res) * weight + bias (the post-norm step of an encoder block)."""
    return _AddLayerNorm.apply(x, res, weight, bias, eps)


# ---------------------------------------------------------------------------------------------
# the recurrent agent's LSTM (ppo_atari_lstm.py:140-158: one nn.LSTM call per step, state * (1 - done))
# ---------------------------------------------------------------------------------------------
LSTM_HIDDEN = (32, 64, 128)


def lstm_shape_ok(T: int, B: int, I: int, H: int) -> bool:
    """The contract of ocppo_lstm_seq_fwd / _bwd / ocppo_lstm_step."""
    return T >= 1 and B >= 1 and I >= 1 and H in LSTM_HIDDEN


def _lstm_shape(pre, w_hh, who: str):
    if pre.dim() != 3 or pre.shape[2] % 4:
        raise ValueError(f"{who}: pre must be [T, B, 4H], got {tuple(pre.shape)}")
    T, B, G = pre.shape
    if not lstm_shape_ok(T, B, 1, G // 4):
        raise ValueError(f"{who}: unsupported T={T} B={B} H={G // 4} (lstm_shape_ok)")
    return T, B, G // 4


def lstm_seq_fwd(pre, w_hh, b_hh, done, h0, c0, save: bool = True):
    """The masked recurrence over pre [T, B, 4H] (= x W_ih^T + b_ih), done [T, B], h0 / c0 [B, H]:
    (h_out [T, B, H], hT, cT [B, H], saved) with saved = (c_out, gates, h_in) for lstm_seq_bwd, or
    None (save=False: inference)."""
    T, B, H = _lstm_shape(pre, w_hh, "lstm_seq_fwd")
    dev, f = pre.device, torch.float32
    h_out = torch.empty((T, B, H), dtype=f, device=dev)
    hT, cT = torch.empty((B, H), dtype=f, device=dev), torch.empty((B, H), dtype=f, device=dev)
    saved = (torch.empty((T, B, H), dtype=f, device=dev),
             torch.empty((T, B, 4 * H), dtype=f, device=dev),
             torch.empty((T, B, H), dtype=f, device=dev)) if save else None
    call("ocppo_lstm_seq_fwd", _stream(dev), _check(pre, "pre", f, dev),
         _check(w_hh, "w_hh", f, dev, 4 * H * H), _check(b_hh, "b_hh", f, dev, 4 * H),
         _check(done, "done", f, dev, T * B), _check(h0, "h0", f, dev, B * H),
         _check(c0, "c0", f, dev, B * H), T, B, H, h_out.data_ptr(),
         *((t.data_ptr() for t in saved) if save else (None, None, None)), hT.data_ptr(),
         cT.data_ptr())
    return h_out, hT, cT, saved


def lstm_seq_bwd(dh_out, gates, c_out, c0, done, w_hh):
    """dgates [T, B, 4H]: the gradient at the pre-activations (= d pre) of lstm_seq_fwd."""
    T, B, H = _lstm_shape(gates, w_hh, "lstm_seq_bwd")
    dev, f = gates.device, torch.float32
    dgates = torch.empty((T, B, 4 * H), dtype=f, device=dev)
    call("ocppo_lstm_seq_bwd", _stream(dev), _check(dh_out, "dh_out", f, dev, T * B * H),
         _check(gates, "gates", f, dev), _check(c_out, "c_out", f, dev, T * B * H),
         _check(c0, "c0", f, dev, B * H), _check(done, "done", f, dev, T * B),
         _check(w_hh, "w_hh", f, dev, 4 * H * H), T, B, H, dgates.data_ptr())
    return dgates


def _lstm_dw_splits(T: int) -> int:
    """Groups of time steps dW_hh = dgates^T h_in is summed over before the groups are added: T
    itself up to 32 steps, else T's largest divisor <= 32."""
    return next(s for s in range(min(T, 32), 0, -1) if T % s == 0)


class _LSTMSeq(torch.autograd.Function):
    """h_out, hT, cT of the masked recurrence; backward = ocppo_lstm_seq_bwd (dpre) + the two
    GEMM-shaped parameter gradients: dW_hh = dgates^T h_in (summed per group of steps), db_hh = the
    column sum of dgates -- written into the flat gradient buffer in place for FlatAdam-owned
    parameters, as agents._LinearAct does. The initial state gets no gradient (the script passes a
    detached clone, ppo_atari_lstm.py:234, 310); hT / cT are not differentiable."""

    @staticmethod
    def forward(ctx, pre, w_hh, b_hh, done, h0, c0):
        pre, w, b = pre.detach().contiguous(), w_hh.detach(), b_hh.detach()
        done, h0, c0 = done.detach().contiguous(), h0.detach().contiguous(), c0.detach().contiguous()
        h_out, hT, cT, (c_out, gates, h_in) = lstm_seq_fwd(pre, w, b, done, h0, c0)
        ctx.save_for_backward(gates, c_out, h_in, c0, done, w)
        ctx.w_hh, ctx.b_hh = w_hh, b_hh
        ctx.mark_non_differentiable(hT, cT)
        return h_out, hT, cT

    @staticmethod
    def backward(ctx, g, _ghT, _gcT):
        from . import agents  # (agents imports this module)

        gates, c_out, h_in, c0, done, w = ctx.saved_tensors
        T, B, G = gates.shape
        dgates = lstm_seq_bwd(g.contiguous(), gates, c_out, c0, done, w)
        dg2 = dgates.view(T * B, G)
        dw = db = None
        if ctx.needs_input_grad[1]:
            # per group of steps first, then over the groups (one bmm + one sum): autograd's own
            # accumulation over the steps of the torch loop has this shape, and a single sum over
            # all T * B rows (agents._weight_grad at these row counts) measured 4x its error
            # (4.8e-7 against 1.2e-7 of the largest element at T * B = 119, H = 128)
            out = ctx.w_hh.grad if agents._direct(ctx.w_hh) else None
            s = _lstm_dw_splits(T)
            part = torch.bmm(dgates.view(s, T // s * B, G).transpose(1, 2),
                             h_in.view(s, T // s * B, G // 4))
            dw = None if out is not None else part.sum(0)
            if out is not None:
                torch.sum(part, 0, out=out)
        if ctx.needs_input_grad[2]:
            if agents._direct(ctx.b_hh):
                torch.sum(dg2, 0, out=ctx.b_hh.grad)
            else:
                db = dg2.sum(0)
        return (dgates if ctx.needs_input_grad[0] else None), dw, db, None, None, None


def lstm_seq(pre, w_hh, b_hh, done, h0, c0):
    """(h_out [T, B, H], (hT, cT)) of Agent.get_states' loop (ppo_atari_lstm.py:148-156) on
    pre = x W_ih^T + b_ih [T, B, 4H]: one launch forward, one backward."""
    for t, name in ((pre, "pre"), (w_hh, "w_hh"), (b_hh, "b_hh"), (done, "done"), (h0, "h0"),
                    (c0, "c0")):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise ValueError(f"lstm_seq: {name} must be a GPU tensor (no CPU fallback)")
    h_out, hT, cT = _LSTMSeq.apply(pre, w_hh, b_hh, done, h0, c0)
    return h_out, (hT, cT)


def lstm_step(x, w_ih, b_ih, w_hh, b_hh, done, h, c):
    """One rollout step (ppo_atari_lstm.py:248, 268): x [N, I], done [N]; h, c [N, H] updated in
    place (and returned). One launch, no autograd."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not isinstance(h, torch.Tensor) or \
            h.dim() != 2:
        raise ValueError("lstm_step: x must be [N, I] and h [N, H]")
    N, I = x.shape
    H = h.shape[1]
    dev, f = x.device, torch.float32
    px = _check(x, "x", f)
    if h.shape[0] != N or not lstm_shape_ok(1, N, I, H):
        raise ValueError(f"lstm_step: unsupported N={N} I={I} H={H} (lstm_shape_ok)")
    call("ocppo_lstm_step", _stream(dev), px, _check(w_ih, "w_ih", f, dev, 4 * H * I),
         _check(b_ih, "b_ih", f, dev, 4 * H), _check(w_hh, "w_hh", f, dev, 4 * H * H),
         _check(b_hh, "b_hh", f, dev, 4 * H), _check(done, "done", f, dev, N), N, I, H,
         _check(h, "h", f, dev, N * H), _check(c, "c", f, dev, N * H))
    return h, c


# ---------------------------------------------------------------------------------------------
# PQN (pqn_atari_envpool.py): Q(lambda), LayerNorm + ReLU, the Q head's acting step, the MSE loss
# on the taken action and RAdam over the flat buffers (csrc/ocppo_pqn.hip, ocppo_optim.hip)
# ---------------------------------------------------------------------------------------------
LN_RELU_MAX_E = 1024
PQN_MAX_ACTIONS, PQN_MAX_HIDDEN = 18, 1024


def q_lambda(rewards, values, dones, next_q, next_done, gamma: float, q_lambda: float,
             returns=None):
    """The Q(lambda) targets of pqn_atari_envpool.py:248-261, bitwise the script's f32 loop:
    rewards / values / dones [T, N] (values = the greedy Q stored at each step), next_q [N, A] =
    q_network(next_obs), next_done [N] -> returns [T, N]."""
    if rewards.dim() != 2 or next_q.dim() != 2:
        raise ValueError(f"q_lambda: rewards must be [T, N] and next_q [N, A], got "
                         f"{tuple(rewards.shape)}, {tuple(next_q.shape)}")
    T, N = rewards.shape
    A = next_q.shape[1]
    dev, f = rewards.device, torch.float32
    if returns is None:
        returns = torch.empty_like(rewards)
    call("ocppo_q_lambda", _stream(dev), _check(rewards, "rewards", f, dev),
         _check(values, "values", f, dev, T * N), _check(dones, "dones", f, dev, T * N),
         _check(next_q, "next_q", f, dev, N * A), _check(next_done, "next_done", f, dev, N), T, N,
         A, float(gamma), float(q_lambda), _check(returns, "returns", f, dev, T * N))
    return returns


def ln_relu_fwd(x, weight, bias, eps: float = 1e-5, relu: bool = True):
    """relu(LayerNorm(x) * weight + bias) over the last dim (relu=False: plain LayerNorm) ->
    (y, mean [R], rstd [R])."""
    return _ln_fwd("ocppo_ln_relu_fwd", x, None, weight, bias, eps, LN_RELU_MAX_E,
                   (int(bool(relu)),))


def ln_relu_bwd(dy, x, y, weight, mean, rstd, relu: bool = True):
    """(dx, dweight, dbias) of ln_relu_fwd; the ReLU mask is y > 0 (y is not read with
    relu=False). The partials live in one buffer per size: every call writes all the partials it
    reads, launches of a stream run one after another."""
    return _ln_bwd("ocppo_ln_relu_bwd",
                   lambda nb, dev: _persistent("ln_relu_bwd", dev, nb, lambda: torch.empty(
                       max(nb // 4, 1), dtype=torch.float32, device=dev)),
                   dy, x, weight, mean, rstd, LN_RELU_MAX_E, y=y if relu else None,
                   flags=(int(bool(relu)),))


class _LnRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps: float, relu: bool):
        x, w = x.detach().contiguous(), weight.detach()
        y, mean, rstd = ln_relu_fwd(x, w, bias.detach(), eps, relu)
        ctx.save_for_backward(x, y, w, mean, rstd)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, g):
        x, y, w, mean, rstd = ctx.saved_tensors
        dx, dw, db = timed("ln_relu_bwd", lambda: ln_relu_bwd(g.contiguous(), x, y, w, mean, rstd,
                                                              ctx.relu))
        return dx, dw, db, None, None


def ln_relu(x, weight, bias, eps: float = 1e-5, relu: bool = True):
    """Differentiable relu(LayerNorm(x) * weight + bias) over the last dim: the LayerNorm -> ReLU
    after every Linear of pqn_atari_envpool.py's QNetwork as one launch (two in the backward)."""
    return _LnRelu.apply(x, weight, bias, eps, relu)


def pqn_act_ok(hidden, wq) -> bool:
    """pqn_act applies: GPU f32 [N, H] rows and an [A, H] head with A <= 18, H a multiple of 4 up
    to 1024, both contiguous and 16-B aligned (q_head_epsilon_greedy's contract, widened)."""
    if not (isinstance(hidden, torch.Tensor) and isinstance(wq, torch.Tensor) and hidden.is_cuda
            and wq.is_cuda and hidden.dtype == wq.dtype == torch.float32 and hidden.dim() == 2
            and wq.dim() == 2):
        return False
    H, A = hidden.shape[1], wq.shape[0]
    return (wq.shape[1] == H and 1 <= A <= PQN_MAX_ACTIONS and 4 <= H <= PQN_MAX_HIDDEN
            and H % 4 == 0 and hidden.is_contiguous() and wq.is_contiguous()
            and (hidden.data_ptr() | wq.data_ptr()) % 16 == 0)


def pqn_act(hidden, wq, bq, seed: int, step, start_e: float, end_e: float, duration: float,
            actions_out=None, values_out=None, epsilon_out=None, step_offset: int = 0, q_out=None):
    """The acting step of pqn_atari_envpool.py:224-232 in one launch: q = hidden @ wq.T + bq,
    values = q's maximum (first index among equal maxima), actions = epsilon_greedy(q, ...)'s
    for the same seed and step. Returns (actions, values)."""
    if not pqn_act_ok(hidden, wq):
        raise ValueError(f"pqn_act: hidden {tuple(getattr(hidden, 'shape', ()))}, wq "
                         f"{tuple(getattr(wq, 'shape', ()))} outside pqn_act_ok")
    N, H = hidden.shape
    A = wq.shape[0]
    dev, f = hidden.device, torch.float32
    if actions_out is None:
        actions_out = torch.empty(N, dtype=torch.int64, device=dev)
    if values_out is None:
        values_out = torch.empty(N, dtype=f, device=dev)
    call("ocppo_pqn_act", _stream(dev), hidden.data_ptr(), N, H, wq.data_ptr(),
         _check(bq, "bq", f, dev, A), A, int(seed) & 0xFFFFFFFFFFFFFFFF,
         _check(step, "step", torch.int64, dev, 1), int(step_offset), float(start_e), float(end_e),
         float(duration), _check(actions_out, "actions", torch.int64, dev, N),
         _check(values_out, "values", f, dev, N), _opt(epsilon_out, "epsilon_out", f, dev, 1),
         _opt(q_out, "q_out", f, dev, N * A))
    return actions_out, values_out


def pqn_loss_fwd_bwd(q, actions, returns, dq=None, stats=None):
    """F.mse_loss(returns, q.gather(1, actions)) of pqn_atari_envpool.py:276-277 with its
    gradient: (stats [2] = {td_loss, mean q(s, a)}, dq [M, A])."""
    if q.dim() != 2 or not 1 <= q.shape[1] <= PQN_MAX_ACTIONS:
        raise ValueError(f"pqn_loss_fwd_bwd: q must be [M, A <= {PQN_MAX_ACTIONS}], got "
                         f"{tuple(q.shape)}")
    M, A = q.shape
    dev, f = q.device, torch.float32
    pq = _check(q, "q", f)
    if dq is None:
        dq = torch.empty_like(q)
    if stats is None:
        stats = torch.empty(2, dtype=f, device=dev)
    call("ocppo_pqn_loss_fwd_bwd", _stream(dev), pq,
         _check(actions, "actions", torch.int64, dev, M), _check(returns, "returns", f, dev, M),
         M, A, _check(dq, "dq", f, dev, M * A), _check(stats, "stats", f, dev, 2))
    return stats, dq


class FlatRAdam(FlatAdam):
    """torch.optim.RAdam (betas (0.9, 0.999), eps 1e-8, no weight decay) + global-norm gradient
    clipping over FlatAdam's flat buffers and views: the same clip and norm kernel, the step is
    ocppo_clip_radam_step (rectification from the device step count; graph-capturable)."""

    ENTRY = "ocppo_clip_radam_step"
    NO_PLANES = ("FlatRAdam writes no weight planes (ocppo_clip_radam_step takes no plane jobs)",
                 (0,))


# ---------------------------------------------------------------------------------------------
# Recurrent PQN (pqn_atari_envpool_lstm.py): the LSTM step + acting step in one launch, and the
# update's Q head + MSE loss + head backward in one call (csrc/ocppo_pqn_lstm.hip)
# ---------------------------------------------------------------------------------------------
def pqn_lstm_act_ok(x, h, wq) -> bool:
    """pqn_lstm_act applies: GPU f32 contiguous x [N, I], h [N, H] with (N, I, H) inside
    lstm_shape_ok, and a contiguous 16-B aligned head wq [A, H] with 1 <= A <= 18."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and
               t.dim() == 2 and t.is_contiguous() for t in (x, h, wq)):
        return False
    (N, I), H, A = x.shape, h.shape[1], wq.shape[0]
    return (h.shape[0] == N and wq.shape[1] == H and lstm_shape_ok(1, N, I, H) and
            1 <= A <= PQN_MAX_ACTIONS and wq.data_ptr() % 16 == 0)


def pqn_lstm_act(x, w_ih, b_ih, w_hh, b_hh, done, h, c, wq, bq, seed: int, step, start_e: float,
                 end_e: float, duration: float, actions_out=None, values_out=None,
                 epsilon_out=None, step_offset: int = 0, q_out=None, commit: bool = True):
    """The rollout step of pqn_atari_envpool_lstm.py:261-267 in one launch: lstm_step on (x, done,
    h, c), then pqn_act on the new h -- bitwise those two calls. commit=True updates h / c in
    place and returns (actions, values); commit=False leaves h / c untouched (the bootstrap of
    :287): no action is drawn (actions_out is not written unless given), returns (None or
    actions_out, values)."""
    if not pqn_lstm_act_ok(x, h, wq):
        raise ValueError(f"pqn_lstm_act: x {tuple(getattr(x, 'shape', ()))}, h "
                         f"{tuple(getattr(h, 'shape', ()))}, wq {tuple(getattr(wq, 'shape', ()))} "
                         f"outside pqn_lstm_act_ok")
    (N, I), H, A = x.shape, h.shape[1], wq.shape[0]
    dev, f = x.device, torch.float32
    if actions_out is None and commit:
        actions_out = torch.empty(N, dtype=torch.int64, device=dev)
    if values_out is None:
        values_out = torch.empty(N, dtype=f, device=dev)
    call("ocppo_pqn_lstm_act", _stream(dev), x.data_ptr(), _check(w_ih, "w_ih", f, dev, 4 * H * I),
         _check(b_ih, "b_ih", f, dev, 4 * H), _check(w_hh, "w_hh", f, dev, 4 * H * H),
         _check(b_hh, "b_hh", f, dev, 4 * H), _check(done, "done", f, dev, N), N, I, H,
         h.data_ptr(), _check(c, "c", f, dev, N * H), int(bool(commit)), wq.data_ptr(),
         _check(bq, "bq", f, dev, A), A, int(seed) & 0xFFFFFFFFFFFFFFFF,
         _check(step, "step", torch.int64, dev, 1), int(step_offset), float(start_e), float(end_e),
         float(duration), _opt(actions_out, "actions", torch.int64, dev, N),
         _check(values_out, "values", f, dev, N), _opt(epsilon_out, "epsilon_out", f, dev, 1),
         _opt(q_out, "q_out", f, dev, N * A))
    return actions_out, values_out


PQN_HEAD_LOSS_MAX_H = 1024


def pqn_head_loss_ok(h, wq) -> bool:
    """pqn_head_loss_fwd_bwd applies: GPU f32 contiguous 16-B aligned h [M >= 1, H] and wq [A, H]
    with H a multiple of 4 in [4, 1024] and 1 <= A <= 18."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and
               t.dim() == 2 and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (h, wq)):
        return False
    (M, H), A = h.shape, wq.shape[0]
    return (wq.shape[1] == H and M >= 1 and 4 <= H <= PQN_HEAD_LOSS_MAX_H and H % 4 == 0 and
            1 <= A <= PQN_MAX_ACTIONS)


class HeadLossWorkspace:
    """Device scratch of pqn_head_loss_fwd_bwd for one (M, H, A): the per-workgroup partials (no
    initial contents needed) behind the rows' q_a, which every call leaves in `q_taken`."""

    def __init__(self, M: int, H: int, A: int, device):
        self.nbytes = int(_lib.LIB.ocppo_pqn_head_loss_workspace_bytes(M, H, A))
        if self.nbytes == 0:
            raise ValueError(f"HeadLossWorkspace: M={M} H={H} A={A} outside the contract")
        self.buf = torch.zeros(self.nbytes // 4, dtype=torch.float32, device=device)
        self.M, self.H, self.A = M, H, A

    @property
    def q_taken(self):
        """q_a [M] of the last call: h[m] . wq[a_m] + bq[a_m]."""
        return self.buf[:self.M]


def pqn_head_loss_fwd_bwd(h, wq, bq, actions, returns, dh=None, dwq=None, dbq=None, stats=None,
                          workspace: HeadLossWorkspace | None = None):
    """The update's Q head, F.mse_loss(returns, q.gather(1, actions)) and the head's backward of
    pqn_atari_envpool_lstm.py:318-325 in one call, from the head's input h [M, H]:
    (stats [2] = {td_loss, mean q(s, a)}, dh [M, H], dwq [A, H], dbq [A]); dwq / dbq are
    overwritten (point them at the head's .grad views)."""
    if not pqn_head_loss_ok(h, wq):
        raise ValueError(f"pqn_head_loss_fwd_bwd: h {tuple(getattr(h, 'shape', ()))}, wq "
                         f"{tuple(getattr(wq, 'shape', ()))} outside pqn_head_loss_ok")
    (M, H), A = h.shape, wq.shape[0]
    dev, f = h.device, torch.float32
    if dh is None:
        dh = torch.empty_like(h)
    if dwq is None:
        dwq = torch.empty_like(wq)
    if dbq is None:
        dbq = torch.empty(A, dtype=f, device=dev)
    if stats is None:
        stats = torch.empty(2, dtype=f, device=dev)
    if workspace is None:
        workspace = HeadLossWorkspace(M, H, A, dev)
    if (workspace.M, workspace.H, workspace.A) != (M, H, A) or workspace.buf.device != dev:
        raise ValueError(f"pqn_head_loss_fwd_bwd: workspace of {(workspace.M, workspace.H, workspace.A)}"
                         f" for M, H, A = {(M, H, A)}")
    call("ocppo_pqn_head_loss_fwd_bwd", _stream(dev), h.data_ptr(), wq.data_ptr(),
         _check(bq, "bq", f, dev, A), _check(actions, "actions", torch.int64, dev, M),
         _check(returns, "returns", f, dev, M), M, H, A, _check(dh, "dh", f, dev, M * H),
         _check(dwq, "dwq", f, dev, A * H), _check(dbq, "dbq", f, dev, A),
         _check(stats, "stats", f, dev, 2), workspace.buf.data_ptr(), workspace.nbytes)
    return stats, dh, dwq, dbq


# ---------------------------------------------------------------------------------------------
# Discrete SAC (sac_atari.py): acting, twin soft-Q loss, policy + temperature loss and its Adam
# ---------------------------------------------------------------------------------------------
SAC_MAX_ACTIONS = C51_MAX_ACTIONS


def _sac_shape(x, name: str):
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not 1 <= x.shape[1] <= SAC_MAX_ACTIONS:
        raise ValueError(f"{name} must be [rows, A <= {SAC_MAX_ACTIONS}], got "
                         f"{tuple(getattr(x, 'shape', ()))}")
    return x.shape


def sac_act(logits, seed: int, step, learning_starts: int, actions_out=None,
            step_offset: int = 0):
    """sac_atari.py:248-252 in one launch: at t = step + step_offset < learning_starts a uniform
    action per env, otherwise one draw of Categorical(logits) (the exponential race, first
    maximum); the library's counter stream under the SAC key, keyed by (seed, t, env, j)."""
    E, A = _sac_shape(logits, "sac_act: logits")
    dev = logits.device
    if actions_out is None:
        actions_out = torch.empty(E, dtype=torch.int64, device=dev)
    call("ocppo_sac_act", _stream(dev), _check(logits, "logits", torch.float32, dev), E, A,
         int(seed) & 0xFFFFFFFFFFFFFFFF, _check(step, "step", torch.int64, dev, 1),
         int(step_offset), int(learning_starts),
         _check(actions_out, "actions", torch.int64, dev, E))
    return actions_out


def sac_critic_loss_fwd_bwd(next_logits, q1_next_target, q2_next_target, q1, q2, actions, rewards,
                            dones, gamma: float, alpha, dq1=None, dq2=None, stats=None, y=None):
    """sac_atari.py:283-302 in one launch: the soft target from the actor's logits and the two
    target critics on the next observations, both MSE losses and d loss / d q1, d loss / d q2.
    alpha: a device f32 scalar. Returns (stats [4] = {qf1_loss, qf2_loss, mean q1(s, a),
    mean q2(s, a)}, dq1, dq2); y [B], if given, receives the targets."""
    B, A = _sac_shape(q1, "sac_critic_loss_fwd_bwd: q1")
    dev, f = q1.device, torch.float32
    n = B * A
    if dq1 is None:
        dq1 = torch.empty_like(q1)
    if dq2 is None:
        dq2 = torch.empty_like(q1)
    if stats is None:
        stats = torch.empty(4, dtype=f, device=dev)
    call("ocppo_sac_critic_loss_fwd_bwd", _stream(dev),
         _check(next_logits, "next_logits", f, dev, n),
         _check(q1_next_target, "q1_next_target", f, dev, n),
         _check(q2_next_target, "q2_next_target", f, dev, n), _check(q1, "q1", f, dev, n),
         _check(q2, "q2", f, dev, n), _check(actions, "actions", torch.int64, dev, B),
         _check(rewards, "rewards", f, dev, B), _check(dones, "dones", f, dev, B), B, A,
         float(gamma), _check(alpha, "alpha", f, dev, 1), _check(dq1, "dq1", f, dev, n),
         _check(dq2, "dq2", f, dev, n), _check(stats, "stats", f, dev, 4),
         _opt(y, "y", f, dev, B))
    return stats, dq1, dq2


class FlatAdamExact(FlatAdam):
    """FlatAdam with torch.optim.Adam's step scalars formed as torch forms them, in double
    (ocppo_clip_adam_step_exact): a bias that starts at zero then follows torch's to f32 rounding,
    where FlatAdam's f32 `1 - beta^t` leaves up to 6e-7 of every step. FlatAdam itself (and what
    the other learners compute) is unchanged. No weight planes."""

    ENTRY = "ocppo_clip_adam_step_exact"
    NO_PLANES = ("FlatAdamExact writes no weight planes", ())


class SacTemperature:
    """The temperature of sac_atari.py:227-233 on the device: alpha, log_alpha and, with
    autotune, log_alpha's Adam state (torch.optim.Adam([log_alpha], lr, eps=1e-4): exp_avg,
    exp_avg_sq, step). sac_actor_alpha_fwd_bwd updates it in its launch."""

    def __init__(self, device, autotune: bool, alpha: float, lr: float, target_entropy: float,
                 betas=(0.9, 0.999), eps: float = 1e-4):
        dev, f = torch.device(device), torch.float32
        self.autotune = bool(autotune)
        self.log_alpha = torch.zeros(1, dtype=f, device=dev)
        # autotune: alpha = log_alpha.exp() = 1 (:229-230), else the flag's value
        self.alpha = torch.full((1,), 1.0 if autotune else float(alpha), dtype=f, device=dev)
        self.exp_avg = torch.zeros(1, dtype=f, device=dev)
        self.exp_avg_sq = torch.zeros(1, dtype=f, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.target_entropy = float(target_entropy)


def sac_actor_alpha_fwd_bwd(logits, q1, q2, temp: SacTemperature, dlogits=None, stats=None):
    """sac_atari.py:309-328 in one launch: the policy loss and d loss / d logits, the temperature
    loss and, with temp.autotune, log_alpha's Adam step and alpha = exp(log_alpha) (read by the
    next critic launch). Returns (stats [4] = {actor_loss, alpha_loss, alpha, mean entropy},
    dlogits)."""
    B, A = _sac_shape(logits, "sac_actor_alpha_fwd_bwd: logits")
    dev, f = logits.device, torch.float32
    n = B * A
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    if stats is None:
        stats = torch.empty(4, dtype=f, device=dev)
    call("ocppo_sac_actor_alpha_fwd_bwd", _stream(dev), _check(logits, "logits", f, dev, n),
         _check(q1, "q1", f, dev, n), _check(q2, "q2", f, dev, n), B, A,
         _check(temp.alpha, "alpha", f, dev, 1), _check(temp.log_alpha, "log_alpha", f, dev, 1),
         temp.target_entropy, _check(temp.exp_avg, "exp_avg", f, dev, 1),
         _check(temp.exp_avg_sq, "exp_avg_sq", f, dev, 1),
         _check(temp.step, "adam_step", torch.int64, dev, 1), temp.lr, temp.betas[0],
         temp.betas[1], temp.eps, int(temp.autotune), _check(dlogits, "dlogits", f, dev, n),
         _check(stats, "stats", f, dev, 4))
    return stats, dlogits


# ---------------------------------------------------------------------------------------------
# Random Network Distillation (ppo_rnd_envpool.py): running statistics, normalisation, curiosity,
# reward filter, both GAE scans, intrinsic value + masked forward loss (csrc/ocppo_rnd.hip)
# ---------------------------------------------------------------------------------------------
def rms_state(C: int, device):
    """gym's RunningMeanStd(shape=[C]) on the device: f64 [2C + 1] = mean (zeros), var (ones),
    count (1e-4)."""
    st = torch.zeros(2 * C + 1, dtype=torch.float64, device=device)
    st[C:2 * C] = 1.0
    st[2 * C] = 1e-4
    return st


def _rows2d(x, name: str):
    """(pointer, dtype code, R, C, row stride) of x [R, C] f32 / bf16 / u8 on the GPU whose rows
    are contiguous and a fixed number of elements apart (a frame of a stacked observation)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.device.type != "cuda":
        raise ValueError(f"{name}: expected a GPU tensor [R, C], got "
                         f"{tuple(getattr(x, 'shape', ()))} on {getattr(x, 'device', None)}")
    if x.dtype not in _DTYPE_CODE:
        raise ValueError(f"{name}: dtype {x.dtype}, expected float32, bfloat16 or uint8")
    R, C = x.shape
    if R < 1 or C < 1:
        raise ValueError(f"{name}: empty [{R}, {C}]")
    ld = x.stride(0) if R > 1 else C
    if (C > 1 and x.stride(1) != 1) or ld < C:
        raise ValueError(f"{name}: rows must be contiguous and at least C elements apart, got "
                         f"strides {x.stride()}")
    return x.data_ptr(), _DTYPE_CODE[x.dtype], R, C, ld


def _rnd_ws(tag: str, dev, nbytes: int):
    return _persistent(tag, dev, nbytes, lambda: torch.empty(
        max(nbytes // 8, 1), dtype=torch.float64, device=dev))


def rms_update(x, state):
    """gym's RunningMeanStd.update(x) on the device state [2C + 1] f64 (rms_state): the per-column
    batch mean and population variance of x [R, C] (f32 / bf16 / u8, rows possibly strided) merged
    with count R (ppo_rnd_envpool.py:333, :444). Two launches."""
    px, code, R, C, ld = _rows2d(x, "rms_update: x")
    dev = x.device
    nb = int(_lib.LIB.ocppo_rms_update_workspace_bytes(R, C))
    ws = _rnd_ws("rms_update", dev, nb)
    call("ocppo_rms_update", _stream(dev), px, code, R, C, ld,
         _check(state, "state", torch.float64, dev, 2 * C + 1), ws.data_ptr(), ws.numel() * 8)
    return state


def rnd_normalize(x, state, out=None):
    """((x - mean) / sqrt(var)).clip(-5, 5).float() of ppo_rnd_envpool.py:365-370 / :449-454 with
    the f64 statistics of rms_update: out [R, C] f32."""
    px, code, R, C, ld = _rows2d(x, "rnd_normalize: x")
    dev = x.device
    if out is None:
        out = torch.empty((R, C), dtype=torch.float32, device=dev)
    call("ocppo_rnd_normalize", _stream(dev), px, code, R, C, ld,
         _check(state, "state", torch.float64, dev, 2 * C + 1),
         _check(out, "out", torch.float32, dev, R * C))
    return out


def rnd_curiosity(pred, target, out=None):
    """(target - pred).pow(2).sum(1) / 2 of ppo_rnd_envpool.py:373; rows [R, D] f32 -> [R]."""
    if pred.dim() != 2 or pred.shape[1] < 1:
        raise ValueError(f"rnd_curiosity: pred must be [R, D >= 1], got {tuple(pred.shape)}")
    R, D = pred.shape
    dev, f = pred.device, torch.float32
    pp = _check(pred, "pred", f)
    if out is None:
        out = torch.empty(R, dtype=f, device=dev)
    call("ocppo_rnd_error", _stream(dev), pp, _check(target, "target", f, dev, R * D), R, D,
         _check(out, "out", f, dev, R))
    return out


def rnd_reward_norm(curiosity, rewems, state, int_gamma: float, filtered=None):
    """ppo_rnd_envpool.py:390-400 in two launches: the RewardForwardFilter over curiosity [T, N]
    along the env axis (rewems [T] f32 carried across calls, zeros at first), the filtered values'
    mean and population variance merged into state [3] f64 = {mean, var, count} with count N, and
    curiosity /= f32(sqrt(var)) in place. filtered [N, T], if given, receives the filter output."""
    if curiosity.dim() != 2:
        raise ValueError(f"rnd_reward_norm: curiosity must be [T, N], got {tuple(curiosity.shape)}")
    T, N = curiosity.shape
    dev, f = curiosity.device, torch.float32
    pc = _check(curiosity, "curiosity", f)
    nb = int(_lib.LIB.ocppo_rnd_reward_norm_workspace_bytes(T))
    ws = _rnd_ws("rnd_reward_norm", dev, nb)
    call("ocppo_rnd_reward_norm", _stream(dev), pc, _check(rewems, "rewems", f, dev, T),
         _check(state, "state", torch.float64, dev, 3), T, N, float(int_gamma), ws.data_ptr(),
         ws.numel() * 8, _opt(filtered, "filtered", f, dev, T * N))
    return curiosity


def rnd_gae(rewards, ext_values, dones, next_ext_value, next_done, curiosity, int_values,
            next_int_value, gamma: float, int_gamma: float, gae_lambda: float, int_coef: float,
            ext_coef: float, ext_advantages=None, ext_returns=None, int_advantages=None,
            int_returns=None, advantages=None):
    """Both GAE scans of ppo_rnd_envpool.py:406-430 and the combined advantage of :442 in one
    launch, bitwise the script's f32 loop: [T, N] f32 in, (ext_adv, ext_ret, int_adv, int_ret,
    adv = int_adv * int_coef + ext_adv * ext_coef) out."""
    if rewards.dim() != 2:
        raise ValueError(f"rnd_gae: rewards must be [T, N], got {tuple(rewards.shape)}")
    T, N = rewards.shape
    dev, f = rewards.device, torch.float32
    outs = [torch.empty_like(rewards) if o is None else o
            for o in (ext_advantages, ext_returns, int_advantages, int_returns, advantages)]
    names = ("ext_advantages", "ext_returns", "int_advantages", "int_returns", "advantages")
    call("ocppo_rnd_gae", _stream(dev), _check(rewards, "rewards", f, dev),
         _check(ext_values, "ext_values", f, dev, T * N), _check(dones, "dones", f, dev, T * N),
         _check(next_ext_value, "next_ext_value", f, dev, N),
         _check(next_done, "next_done", f, dev, N),
         _check(curiosity, "curiosity", f, dev, T * N),
         _check(int_values, "int_values", f, dev, T * N),
         _check(next_int_value, "next_int_value", f, dev, N), T, N, float(gamma),
         float(int_gamma), float(gae_lambda), float(int_coef), float(ext_coef),
         *[_check(o, n, f, dev, T * N) for o, n in zip(outs, names)])
    return tuple(outs)


RND_STAT_NAMES = ("int_v_loss", "fwd_loss", "mask_count")


def rnd_mask_counter(device):
    """The device minibatch counter of the update mask's stream (i64 [1], zero)."""
    return torch.zeros(1, dtype=torch.int64, device=device)


def rnd_aux_loss_fwd_bwd(pred, target, v_int, ret_int, seed: int, counter,
                         update_proportion: float, vf_coef: float, dpred=None, dv_int=None,
                         stats=None):
    """The intrinsic value loss and the masked forward loss of ppo_rnd_envpool.py:463-472, :509
    with their gradients: dpred [M, D] = d loss / d pred, dv_int [M] = vf_coef * d int_v_loss /
    d v_int, stats [3] = RND_STAT_NAMES. The mask is the library's counter stream keyed by (seed,
    counter, row); counter (rnd_mask_counter) advances by one on the device. Two launches."""
    if pred.dim() != 2 or pred.shape[0] < 1 or pred.shape[1] < 1:
        raise ValueError(f"rnd_aux_loss_fwd_bwd: pred must be [M >= 1, D >= 1], got "
                         f"{tuple(pred.shape)}")
    M, D = pred.shape
    dev, f = pred.device, torch.float32
    pp = _check(pred, "pred", f)
    if dpred is None:
        dpred = torch.empty_like(pred)
    if dv_int is None:
        dv_int = torch.empty(M, dtype=f, device=dev)
    if stats is None:
        stats = torch.empty(3, dtype=f, device=dev)
    nb = int(_lib.LIB.ocppo_rnd_aux_loss_workspace_bytes(M))
    ws = _rnd_ws("rnd_aux_loss_fwd_bwd", dev, nb)
    call("ocppo_rnd_aux_loss_fwd_bwd", _stream(dev), pp, _check(target, "target", f, dev, M * D),
         _check(v_int, "v_int", f, dev, M), _check(ret_int, "ret_int", f, dev, M), M, D,
         int(seed) & 0xFFFFFFFFFFFFFFFF, _check(counter, "counter", torch.int64, dev, 1),
         float(update_proportion), float(vf_coef), _check(dpred, "dpred", f, dev, M * D),
         _check(dv_int, "dv_int", f, dev, M), _check(stats, "stats", f, dev, 3), ws.data_ptr(),
         ws.numel() * 8)
    return stats, dpred, dv_int


def rnd_mask(seed: int, counter, M: int, update_proportion: float, out=None):
    """The update mask rnd_aux_loss_fwd_bwd applies at `counter` (left as it is): f32 0 / 1 [M]."""
    dev = counter.device
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=dev)
    call("ocppo_rnd_mask", _stream(dev), int(seed) & 0xFFFFFFFFFFFFFFFF,
         _check(counter, "counter", torch.int64, dev, 1), M, float(update_proportion),
         _check(out, "out", torch.float32, dev, M))
    return out


# ---------------------------------------------------------------------------------------------
# Phasic Policy Gradient (ppg_procgen.py): the auxiliary minibatch gather, the auxiliary loss with
# its three gradients (csrc/ocppo_ppg.hip) and Adam with a step count per segment
# ---------------------------------------------------------------------------------------------
PPG_MAX_ACTIONS = 18
PPG_STAT_NAMES = ("kl_loss", "aux_value_loss", "real_value_loss")


def ppg_aux_loss_fwd_bwd(new_logits, new_value, new_aux_value, old_logits, returns,
                         beta_clone: float, dlogits=None, dvalue=None, daux=None, stats=None):
    """ppg_procgen.py:449-461 with its gradients: kl_loss = mean KL(Categorical(old_logits) ||
    Categorical(new_logits)), the two value regressions 0.5 mean (v - returns)^2, and the
    gradients of aux_value_loss + beta_clone * kl_loss + real_value_loss: dlogits [M, A] =
    beta_clone / M (p_new - p_old), dvalue [M] = (new_value - returns) / M, daux [M] likewise.
    Returns (stats [3] = PPG_STAT_NAMES, dlogits, dvalue, daux). Two launches."""
    if new_logits.dim() != 2 or new_logits.shape[0] < 1 or \
            not 1 <= new_logits.shape[1] <= PPG_MAX_ACTIONS:
        raise ValueError(f"ppg_aux_loss_fwd_bwd: new_logits must be [M >= 1, 1 <= A <= "
                         f"{PPG_MAX_ACTIONS}], got {tuple(new_logits.shape)}")
    M, A = new_logits.shape
    dev, f = new_logits.device, torch.float32
    pl = _check(new_logits, "new_logits", f)
    if dlogits is None:
        dlogits = torch.empty_like(new_logits)
    if dvalue is None:
        dvalue = torch.empty(M, dtype=f, device=dev)
    if daux is None:
        daux = torch.empty(M, dtype=f, device=dev)
    if stats is None:
        stats = torch.empty(3, dtype=f, device=dev)
    nb = int(_lib.LIB.ocppo_ppg_aux_loss_workspace_bytes(M))
    ws = _persistent("ppg_aux_loss_fwd_bwd", dev, nb, lambda: torch.empty(
        max(nb // 8, 1), dtype=torch.float64, device=dev))
    call("ocppo_ppg_aux_loss_fwd_bwd", _stream(dev), pl,
         _check(new_value, "new_value", f, dev, M),
         _check(new_aux_value, "new_aux_value", f, dev, M),
         _check(old_logits, "old_logits", f, dev, M * A), _check(returns, "returns", f, dev, M),
         M, A, float(beta_clone), _check(dlogits, "dlogits", f, dev, M * A),
         _check(dvalue, "dvalue", f, dev, M), _check(daux, "daux", f, dev, M),
         _check(stats, "stats", f, dev, 3), ws.data_ptr(), ws.numel() * 8)
    return stats, dlogits, dvalue, daux


def ppg_aux_gather(aux_obs, aux_pi, aux_returns, cols, out_obs=None, out_pi=None,
                   out_returns=None):
    """The auxiliary minibatch of ppg_procgen.py:443-453 in one launch: flatten01(aux_*[:, cols])
    of aux_obs [T, R, ...] (f32 / bf16 / u8, converted exactly to f32), aux_pi [T, R, A] f32 and
    aux_returns [T, R] f32 -> (out_obs [T k, ...], out_pi [T k, A], out_returns [T k]), rows t
    major. cols: k column indices, an int64 device tensor (graph replays read it afresh; an index
    outside [0, R) is clamped into the range by the kernel, never dereferenced) or a host
    list, which is checked here and refused when out of range."""
    if aux_obs.dim() < 3 or aux_pi.dim() != 3 or aux_returns.dim() != 2:
        raise ValueError("ppg_aux_gather: aux_obs [T, R, ...], aux_pi [T, R, A], aux_returns [T, R]")
    T, R = aux_obs.shape[:2]
    A = aux_pi.shape[2]
    D = aux_obs[0, 0].numel() if T and R else 0
    dev, f = aux_obs.device, torch.float32
    if aux_obs.dtype not in _DTYPE_CODE:
        raise ValueError(f"ppg_aux_gather: unsupported aux_obs dtype {aux_obs.dtype}")
    if tuple(aux_pi.shape[:2]) != (T, R) or tuple(aux_returns.shape) != (T, R) or \
            min(T, R, A, D) < 1:
        raise ValueError(f"ppg_aux_gather: shapes {tuple(aux_obs.shape)}, {tuple(aux_pi.shape)}, "
                         f"{tuple(aux_returns.shape)} do not agree on [T >= 1, R >= 1]")
    if not isinstance(cols, torch.Tensor):
        cols = [int(c) for c in cols]
        bad = [c for c in cols if not 0 <= c < R]
        if bad:
            raise IndexError(f"ppg_aux_gather: column indices {bad} outside [0, {R})")
        cols = torch.tensor(cols, dtype=torch.int64, device=dev)
    k = cols.numel()
    if k < 1:
        raise ValueError("ppg_aux_gather: no columns")
    if out_obs is None:
        out_obs = torch.empty((T * k,) + tuple(aux_obs.shape[2:]), dtype=f, device=dev)
    if out_pi is None:
        out_pi = torch.empty((T * k, A), dtype=f, device=dev)
    if out_returns is None:
        out_returns = torch.empty(T * k, dtype=f, device=dev)
    call("ocppo_ppg_aux_gather", _stream(dev), _check(aux_obs, "aux_obs", None, dev),
         _DTYPE_CODE[aux_obs.dtype], _check(aux_pi, "aux_pi", f, dev),
         _check(aux_returns, "aux_returns", f, dev), _check(cols, "cols", torch.int64, dev, k),
         T, R, k, D, A, _check(out_obs, "out_obs", f, dev, T * k * D),
         _check(out_pi, "out_pi", f, dev, T * k * A),
         _check(out_returns, "out_returns", f, dev, T * k))
    return out_obs, out_pi, out_returns


OPT_TAIL_SKIPPED, OPT_TAIL_STEP = _lib.OCPPO_OPT_TAIL_SKIPPED, _lib.OCPPO_OPT_TAIL_STEP


class FlatAdamSegments(FlatAdam):
    """FlatAdam over a flat buffer of two segments -- `params` (the head) followed by
    `tail_params` -- each with its own device step count, as torch.optim.Adam keeps one per
    parameter and skips a parameter whose grad is None (ocppo_clip_adam_step_seg).
    step(tail_active=False): the clip norm runs over the head's gradients alone and the tail's
    parameters, moments and step count are neither read nor written; step(True): one clip over
    both, each segment's step scalars formed from its own count exactly as FlatAdam forms them.
    scalars[OPT_STEP] is the head's count, scalars[OPT_TAIL_STEP] the tail's (as of its last
    step), scalars[OPT_TAIL_SKIPPED] the steps the tail sat out. No weight planes: a trainer
    refreshes them with ops.WeightPlanes.refresh per minibatch."""

    ENTRY = "ocppo_clip_adam_step_seg"
    NO_PLANES = ("FlatAdamSegments writes no weight planes (ocppo_clip_adam_step_seg takes no "
                 "plane jobs)", ())

    def __init__(self, params, tail_params, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float = 0.0):
        head = [p for p in params if p.requires_grad]
        tail = [p for p in tail_params if p.requires_grad]
        if not head or not tail:
            raise ValueError("FlatAdamSegments needs a non-empty head and a non-empty tail")
        if any(p is q for p in head for q in tail):
            raise ValueError("FlatAdamSegments: a parameter is in both segments")
        super().__init__(head + tail, lr, betas, eps, max_grad_norm)
        _, self.split = flat_offsets(head)
        self.head_params, self.tail_params = head, tail

    @property
    def tail_step(self) -> torch.Tensor:
        """The tail's step count (a device f32 scalar)."""
        return self.scalars[OPT_STEP] - self.scalars[OPT_TAIL_SKIPPED]

    def step(self, tail_active: bool = True, grad_scale: float = 1.0):
        dev = self.params.device
        call(self.ENTRY, _stream(dev), self.params.data_ptr(), self.grads.data_ptr(),
             self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.numel, self.split,
             int(bool(tail_active)), self.lr.data_ptr(), self.betas[0], self.betas[1], self.eps,
             float(grad_scale), self.max_grad_norm, self.scalars.data_ptr(), self.ws.data_ptr(),
             self.ws.numel())


# ---------------------------------------------------------------------------------------------
# QDagger (qdagger_dqn_atari_impalacnn.py): the TD + distillation loss, the episodic-return ring
# ---------------------------------------------------------------------------------------------
QDAGGER_RING = 10  # the script's deque(maxlen=10)


def qdagger_loss_fwd_bwd(q, q_next, q_teacher, actions, rewards, dones, gamma: float,
                         temperature: float, distill_coeff=None, dq=None, stats=None):
    """:303-315 / :412-424 in one launch. distill_coeff: a device f32 scalar, None = 1.0 (the
    offline phase). Returns (stats [5] = {loss, q_loss, distill_loss, mean q(s,a), coeff}, dq)."""
    if not isinstance(q, torch.Tensor) or q.dim() != 2:
        raise ValueError("qdagger_loss_fwd_bwd: q: expected a [B, A] tensor")
    B, A = q.shape
    if not (B >= 1 and 1 <= A <= 1024):
        raise ValueError(f"qdagger_loss_fwd_bwd: B={B} A={A}: need B >= 1 and 1 <= A <= 1024")
    if not temperature > 0:
        raise ValueError(f"qdagger_loss_fwd_bwd: temperature={temperature} must be > 0")
    dev = q.device
    f = torch.float32
    if dq is None:
        dq = torch.empty_like(q)
    if stats is None:
        stats = torch.empty(5, dtype=f, device=dev)
    call("ocppo_qdagger_loss_fwd_bwd", _stream(dev), _check(q, "q", f, dev),
         _check(q_next, "q_next", f, dev, B * A), _check(q_teacher, "q_teacher", f, dev, B * A),
         _check(actions, "actions", torch.int64, dev, B), _check(rewards, "rewards", f, dev, B),
         _check(dones, "dones", f, dev, B), B, A, float(gamma), float(temperature),
         _opt(distill_coeff, "distill_coeff", f, dev, 1), _check(dq, "dq", f, dev, B * A),
         _check(stats, "stats", f, dev, 5))
    return stats, dq


class EpisodeRing:
    """The device state of qdagger_episode_push: the envs' running returns, the 10-slot ring of
    finished returns with its int64 {head, count}, and the coefficient the loss launch reads."""

    def __init__(self, num_envs: int, device):
        dev, f = torch.device(device), torch.float32
        self.run_ret = torch.zeros(num_envs, dtype=f, device=dev)
        self.ring = torch.zeros(QDAGGER_RING, dtype=f, device=dev)
        self.state = torch.zeros(2, dtype=torch.int64, device=dev)
        self.coeff = torch.ones(1, dtype=f, device=dev)

    def returns(self) -> list:
        """The ring's returns, oldest first (one host sync)."""
        head, count = self.state.tolist()
        r = self.ring.tolist()
        return r[:count] if count < QDAGGER_RING else r[head:] + r[:head]


def qdagger_episode_push(reward, done, ring: EpisodeRing, teacher_mean: float):
    """:365, :390 and :408-411 for one env step: the raw reward [E] and done [E] go into the
    running returns, finished episodes into the ring in ascending env order, and ring.coeff
    becomes 1 below 10 episodes, else max(1 - mean(ring) / teacher_mean, 0)."""
    dev = reward.device
    f = torch.float32
    E = reward.numel()
    teacher_mean = float(teacher_mean)
    if teacher_mean == 0 or not math.isfinite(teacher_mean):
        raise ValueError(f"qdagger_episode_push: teacher_mean={teacher_mean} must be finite and "
                         "not 0")
    call("ocppo_qdagger_episode_push", _stream(dev), _check(reward, "reward", f, dev),
         _check(done, "done", f, dev, E), E, _check(ring.run_ret, "run_ret", f, dev, E),
         _check(ring.ring, "ring", f, dev, QDAGGER_RING),
         _check(ring.state, "ring_state", torch.int64, dev, 2), teacher_mean,
         _check(ring.coeff, "coeff_out", f, dev, 1))
    return ring.coeff


# ---------------------------------------------------------------------------------------------
# Continuous-action PPO / RPO (ppo_continuous_action.py, rpo_continuous_action.py): the Gaussian
# head's sample, the fused loss, the wrapper chain and Pendulum-v1 (csrc/ocppo_contppo.hip)
# ---------------------------------------------------------------------------------------------
GAUSS_MAX_ACTIONS = 64


def _gauss_shape(mean, logstd, who: str):
    if mean.dim() != 2 or mean.shape[1] < 1:
        raise ValueError(f"{who}: mean must be [rows, A >= 1], got {tuple(mean.shape)}")
    R, A = mean.shape
    if A > GAUSS_MAX_ACTIONS:
        raise ValueError(f"{who}: A = {A} action dimensions, at most {GAUSS_MAX_ACTIONS}")
    if logstd.numel() != A:
        raise ValueError(f"{who}: logstd has {logstd.numel()} elements, expected A = {A}")
    return R, A


def gauss_head_sample(mean, logstd, z, value_in, action=None, logprob=None, value=None):
    """probs.sample() and log_prob(action).sum(1) of ppo_continuous_action.py:134-141 for mean
    [N, A], logstd [A] (or [1, A]) and standard normal draws z [N, A]: action = z * exp(logstd) +
    mean (bitwise torch's z.mul(std).add(mean)), logprob [N] summed in column order, value [N] =
    value_in. One launch."""
    N, A = _gauss_shape(mean, logstd, "gauss_head_sample")
    dev, f = mean.device, torch.float32
    pm = _check(mean, "mean", f)
    if action is None:
        action = torch.empty_like(mean)
    if logprob is None:
        logprob = torch.empty(N, dtype=f, device=dev)
    if value is None:
        value = torch.empty(N, dtype=f, device=dev)
    call("ocppo_gauss_head_sample", _stream(dev), pm, _check(logstd, "logstd", f, dev, A),
         _check(z, "z", f, dev, N * A), _check(value_in, "value_in", f, dev, N), N, A,
         _check(action, "action", f, dev, N * A), _check(logprob, "logprob", f, dev, N),
         _check(value, "value", f, dev, N))
    return action, logprob, value


def rpo_counter(device):
    """The device update counter of the RPO noise stream (i64 [1], zero)."""
    return torch.zeros(1, dtype=torch.int64, device=device)


def gauss_ppo_loss_fwd_bwd(mean, logstd, new_value, actions, logprobs, advantages, returns,
                           values, *, adv_stats=None, clip_coef: float, ent_coef: float,
                           vf_coef: float, norm_adv: bool, clip_vloss: bool, seed: int = 0,
                           counter=None, mb: int = 0, rpo_alpha: float = 0.0, dmean=None,
                           dvalue=None, dlogstd=None, stats=None):
    """ppo_continuous_action.py:265-300 from the network outputs on, with the backward, in one
    launch: (stats [9] in STAT_NAMES' layout, dmean [M, A], dvalue [M], dlogstd [A]). rpo_alpha >
    0: uniform noise in [-alpha, alpha) is added to the mean before the log-prob
    (rpo_continuous_action.py:138-141), drawn from the library's stream at (seed, counter
    (rpo_counter), mb, row, column) -- rpo_noise returns the same draws."""
    M, A = _gauss_shape(mean, logstd, "gauss_ppo_loss_fwd_bwd")
    dev, f = mean.device, torch.float32
    pm = _check(mean, "mean", f)
    rpo_alpha = float(rpo_alpha)
    if rpo_alpha < 0:
        raise ValueError(f"gauss_ppo_loss_fwd_bwd: rpo_alpha = {rpo_alpha} must not be negative")
    if rpo_alpha > 0 and counter is None:
        raise ValueError("gauss_ppo_loss_fwd_bwd: rpo_alpha > 0 needs the device counter")
    if dmean is None:
        dmean = torch.empty_like(mean)
    if dvalue is None:
        dvalue = torch.empty(M, dtype=f, device=dev)
    if dlogstd is None:
        dlogstd = torch.empty(A, dtype=f, device=dev)
    if stats is None:
        stats = torch.empty(len(STAT_NAMES), dtype=f, device=dev)
    call("ocppo_gauss_ppo_loss_fwd_bwd", _stream(dev), pm, _check(logstd, "logstd", f, dev, A),
         _check(new_value, "new_value", f, dev, M), M, A, _check(actions, "actions", f, dev, M * A),
         _check(logprobs, "logprobs", f, dev, M), _check(advantages, "advantages", f, dev, M),
         _check(returns, "returns", f, dev, M), _check(values, "values", f, dev, M),
         _opt(adv_stats, "adv_stats", f, dev, 2) if norm_adv else None, float(clip_coef),
         float(ent_coef), float(vf_coef), int(bool(norm_adv)), int(bool(clip_vloss)),
         int(seed) & 0xFFFFFFFFFFFFFFFF, _opt(counter, "counter", torch.int64, dev, 1), int(mb),
         rpo_alpha, _check(dmean, "dmean", f, dev, M * A), _check(dvalue, "dvalue", f, dev, M),
         _check(dlogstd, "dlogstd", f, dev, A), _check(stats, "stats", f, dev, len(STAT_NAMES)))
    return stats, dmean, dvalue, dlogstd


def rpo_noise(seed: int, counter, mb: int, M: int, A: int, alpha: float, out=None):
    """The [M, A] draws gauss_ppo_loss_fwd_bwd adds to the mean at (seed, counter, mb)."""
    dev = counter.device
    if not 1 <= A <= GAUSS_MAX_ACTIONS:
        raise ValueError(f"rpo_noise: A = {A}, expected 1..{GAUSS_MAX_ACTIONS}")
    if out is None:
        out = torch.empty((M, A), dtype=torch.float32, device=dev)
    call("ocppo_rpo_noise", _stream(dev), int(seed) & 0xFFFFFFFFFFFFFFFF,
         _check(counter, "counter", torch.int64, dev, 1), int(mb), M, A, float(alpha),
         _check(out, "out", torch.float32, dev, M * A))
    return out


def cont_norm_state(N: int, D: int, device):
    """The wrapper chain's per-env statistics [N, 2D + 5] f64: the observation RunningMeanStd
    (mean [D] zeros, var [D] ones, count 1e-4), the return accumulator (0) and the return
    RunningMeanStd (0, 1, 1e-4)."""
    st = torch.zeros((N, 2 * D + 5), dtype=torch.float64, device=device)
    st[:, D:2 * D] = 1.0
    st[:, 2 * D] = 1e-4
    st[:, 2 * D + 3] = 1.0
    st[:, 2 * D + 4] = 1e-4
    return st


def env_normalize(obs, state, obs_out, reward=None, reward_out=None, final_obs=None,
                  terminated=None, truncated=None, gamma: float = 0.99, norm_obs: bool = True,
                  norm_reward: bool = True):
    """The wrapper chain of ppo_continuous_action.py:96-100 on N envs' raw step outputs (obs
    [N, D], reward [N], terminated / truncated [N] f32, final_obs [N, D] = the terminal
    observations of the done envs) with per-env statistics `state` (cont_norm_state): obs_out
    [N, D], reward_out [N]. reward None: a reset (observation path only). One launch."""
    if obs.dim() != 2 or obs.shape[1] < 1:
        raise ValueError(f"env_normalize: obs must be [N, D >= 1], got {tuple(obs.shape)}")
    N, D = obs.shape
    dev, f = obs.device, torch.float32
    po = _check(obs, "obs", f)
    if (terminated is not None or truncated is not None) and final_obs is None:
        raise ValueError("env_normalize: done flags need final_obs")
    call("ocppo_env_normalize", _stream(dev), po, _opt(final_obs, "final_obs", f, dev, N * D),
         _opt(reward, "reward", f, dev, N), _opt(terminated, "terminated", f, dev, N),
         _opt(truncated, "truncated", f, dev, N), N, D,
         _check(state, "state", torch.float64, dev, N * (2 * D + 5)), int(bool(norm_obs)),
         int(bool(norm_reward)), float(gamma), _check(obs_out, "obs_out", f, dev, N * D),
         _opt(reward_out, "reward_out", f, dev, N))
    return obs_out, reward_out


def pendulum_step(seed: int, actions, state, counters, obs_out, reward_out=None, done_out=None,
                  ep_state=None, final_obs_out=None, norm_state=None, norm_obs: bool = True,
                  norm_reward: bool = True, gamma: float = 0.99):
    """One step (actions [N] or [N, 1] f32 torques) or, with actions None, a reset of N device
    Pendulum-v1 envs (gymnasium 0.28.1 dynamics, ClipAction, TimeLimit 200, same-step auto-reset):
    state [N, 2] f64 and counters [N, 2] i64 in/out, obs_out [N, 3] f32, reward_out / done_out [N]
    f32, final_obs_out [N, 3] the terminal observations. norm_state (cont_norm_state(N, 3)): the
    outputs pass through env_normalize's chain in the same launch."""
    N = obs_out.shape[0]
    dev, f = obs_out.device, torch.float32
    call("ocppo_pendulum_step", _stream(dev), int(seed) & 0xFFFFFFFFFFFFFFFF,
         _opt(actions, "actions", f, dev, N), N, _check(state, "state", torch.float64, dev, 2 * N),
         _check(counters, "counters", torch.int64, dev, 2 * N),
         _check(obs_out, "obs_out", f, dev, 3 * N),
         _opt(final_obs_out, "final_obs_out", f, dev, 3 * N),
         _opt(reward_out, "reward_out", f, dev, N), _opt(done_out, "done_out", f, dev, N),
         _opt(ep_state, "ep_state", f, dev, 5 * N),
         _opt(norm_state, "norm_state", torch.float64, dev, 11 * N), int(bool(norm_obs)),
         int(bool(norm_reward)), float(gamma))


# ---------------------------------------------------------------------------------------------
# TD3 / DDPG (td3_continuous_action.py, ddpg_continuous_action.py): float-action replay, acting,
# the smoothed target action, the critic loss, the actor loss's action and the soft target update
# (csrc/ocppo_td3.hip)
# ---------------------------------------------------------------------------------------------
class ContReplayBuffer:
    """SB3 ReplayBuffer(optimize_memory_usage=False, handle_timeout_termination=False) in HBM for
    float-vector actions (td3_continuous_action.py:191-198): obs, next_obs [size, E, D], actions
    [size, E, A], rewards, dones [size, E], all f32; {pos, full} and the sample counter on the
    device, so add / sample are graph-replayable. A sampled batch is the critics' input:
    obs_act [B, D + A] = cat(observations, actions) and next_obs_act [B, D + A] whose action
    columns td3_target_actions fills; `observations` / `next_observations` / `actions` are views."""

    def __init__(self, size: int, n_envs: int, obs_dim: int, action_dim: int, device,
                 seed: int = 0):
        self.size, self.E, self.D, self.A = int(size), int(n_envs), int(obs_dim), int(action_dim)
        if self.size < 1 or self.E < 1 or self.D < 1 or not 1 <= self.A <= GAUSS_MAX_ACTIONS:
            raise ValueError(f"ContReplayBuffer: size={size} E={n_envs} D={obs_dim} A={action_dim}"
                             f" (all >= 1, A <= {GAUSS_MAX_ACTIONS})")
        dev = self.device = torch.device(device)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        self.obs, self.next_obs = z(self.size, self.E, self.D), z(self.size, self.E, self.D)
        self.actions = z(self.size, self.E, self.A)
        self.rewards, self.dones = z(self.size, self.E), z(self.size, self.E)
        self.state = torch.zeros(2, dtype=torch.int64, device=dev)  # pos, full
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def add(self, obs, next_obs, final_obs, done, actions, rewards, terminated=None,
            carry: bool = False):
        """rb.add(obs, real_next_obs, actions, rewards, terminations) of :226-230: real_next_obs =
        final_obs where done else next_obs. carry: obs <- next_obs afterwards (:233)."""
        dev, f = self.device, torch.float32
        if (final_obs is None) != (done is None):
            raise ValueError("ContReplayBuffer.add: final_obs and done come together")
        n = self.E * self.D
        call("ocppo_cont_replay_add", _stream(dev), _check(obs, "obs", f, dev, n),
             _check(next_obs, "next_obs", f, dev, n), _opt(final_obs, "final_obs", f, dev, n),
             _opt(done, "done", f, dev, self.E), _check(actions, "actions", f, dev, self.E * self.A),
             _check(rewards, "rewards", f, dev, self.E),
             _opt(terminated, "terminated", f, dev, self.E), self.E, self.D, self.A,
             self.state.data_ptr(), self.size, self.obs.data_ptr(), self.next_obs.data_ptr(),
             self.actions.data_ptr(), self.rewards.data_ptr(), self.dones.data_ptr(),
             int(bool(carry)))

    def batch(self, batch_size: int, with_indices: bool = False) -> dict:
        """Output buffers of one sample (and the strided views of them)."""
        B, D, dev = int(batch_size), self.D, self.device
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        out = {"obs_act": z(B, D + self.A), "next_obs_act": z(B, D + self.A),
               "rewards": z(B, 1), "dones": z(B, 1)}
        out["observations"] = out["obs_act"][:, :D]
        out["actions"] = out["obs_act"][:, D:]
        out["next_observations"] = out["next_obs_act"][:, :D]
        if with_indices:
            out["indices"] = torch.zeros((B, 2), dtype=torch.int64, device=dev)
        return out

    def sample(self, batch_size: int, out: dict | None = None, with_indices: bool = False):
        dev, f = self.device, torch.float32
        B = int(batch_size)
        if B < 1:
            raise ValueError(f"ContReplayBuffer.sample: batch_size = {B}")
        if out is None:
            out = self.batch(B, with_indices)
        n = B * (self.D + self.A)
        call("ocppo_cont_replay_sample", _stream(dev), self.seed, self.counter.data_ptr(),
             self.state.data_ptr(), self.size, self.E, self.D, self.A, self.obs.data_ptr(),
             self.next_obs.data_ptr(), self.actions.data_ptr(), self.rewards.data_ptr(),
             self.dones.data_ptr(), B, _check(out["obs_act"], "obs_act", f, dev, n),
             _check(out["next_obs_act"], "next_obs_act", f, dev, n),
             _check(out["rewards"], "rewards", f, dev, B), _check(out["dones"], "dones", f, dev, B),
             _check(out["indices"], "indices", torch.int64, dev, 2 * B) if "indices" in out
             else None)
        return out


def _td3_vec(t, name: str, A: int, dev):
    return _check(t, name, torch.float32, dev, A)


def td3_act(hidden, w_mu, b_mu, action_scale, action_bias, low, high, seed: int, step,
            learning_starts: int, exploration_noise: float, actions_out=None,
            step_offset: int = 0):
    """td3_continuous_action.py:205-211 at global step t = step[0] + step_offset, from the actor's
    last hidden [E, H]: t < learning_starts: uniform in [low, high) per dimension; otherwise
    clip(tanh(hidden @ w_mu.T + b_mu) * scale + bias + (scale * exploration_noise) * z, low, high).
    One launch; the branch is taken on the device. td3_noise returns z (and the uniform u)."""
    if hidden.dim() != 2 or w_mu.dim() != 2 or w_mu.shape[1] != hidden.shape[1]:
        raise ValueError(f"td3_act: hidden {tuple(hidden.shape)} against w_mu {tuple(w_mu.shape)}")
    E, H = hidden.shape
    A = w_mu.shape[0]
    if not 1 <= A <= GAUSS_MAX_ACTIONS:
        raise ValueError(f"td3_act: A = {A} action dimensions, at most {GAUSS_MAX_ACTIONS}")
    dev, f = hidden.device, torch.float32
    if actions_out is None:
        actions_out = torch.empty((E, A), dtype=f, device=dev)
    call("ocppo_td3_act", _stream(dev), _check(hidden, "hidden", f), E, H,
         _check(w_mu, "w_mu", f, dev, A * H), _check(b_mu, "b_mu", f, dev, A), A,
         _td3_vec(action_scale, "action_scale", A, dev), _td3_vec(action_bias, "action_bias", A, dev),
         _td3_vec(low, "low", A, dev), _td3_vec(high, "high", A, dev),
         int(seed) & 0xFFFFFFFFFFFFFFFF, _check(step, "step", torch.int64, dev, 1),
         int(step_offset), int(learning_starts), float(exploration_noise),
         _check(actions_out, "actions", f, dev, E * A))
    return actions_out


def _td3_draws(seed: int, counter, offset: int, rows: int, A: int, mode: int, out):
    dev = counter.device
    if not 1 <= A <= GAUSS_MAX_ACTIONS:
        raise ValueError(f"td3 noise: A = {A}, expected 1..{GAUSS_MAX_ACTIONS}")
    if out is None:
        out = torch.empty((rows, A), dtype=torch.float32, device=dev)
    call("ocppo_td3_noise", _stream(dev), int(seed) & 0xFFFFFFFFFFFFFFFF,
         _check(counter, "counter", torch.int64, dev, 1), int(offset), int(rows), A, mode,
         _check(out, "out", torch.float32, dev, rows * A))
    return out


def td3_noise(seed: int, step, E: int, A: int, step_offset: int = 0, uniform: bool = False,
              out=None):
    """The [E, A] draws td3_act uses at global step step[0] + step_offset: the standard normal z,
    or with `uniform` the random phase's u in [0, 1) (action = low + (high - low) * u)."""
    return _td3_draws(seed, step, step_offset, E, A, 1 if uniform else 0, out)


def td3_target_noise(seed: int, counter, B: int, A: int, offset: int = 0, out=None):
    """The [B, A] standard normal draws td3_target_actions uses at sample counter counter[0] +
    offset (the replay's counter after the sample: offset 0)."""
    return _td3_draws(seed, counter, offset, B, A, 2, out)


def td3_target_actions(mu, action_scale, action_bias, next_obs_act, seed: int = 0, counter=None,
                       policy_noise: float = 0.0, noise_clip: float = 0.0, low: float = 0.0,
                       high: float = 0.0):
    """td3_continuous_action.py:239-245 from the target actor's pre-tanh output mu [B, A], into
    the action columns of next_obs_act [B, D + A]: clamp(tanh(mu) * scale + bias + clamp(z *
    policy_noise, -noise_clip, noise_clip) * scale, low, high) with the scalar bounds of the first
    action dimension. policy_noise == 0 (ddpg_continuous_action.py:216): tanh(mu) * scale + bias."""
    if mu.dim() != 2 or next_obs_act.dim() != 2 or next_obs_act.shape[0] != mu.shape[0] or \
            next_obs_act.shape[1] <= mu.shape[1]:
        raise ValueError(f"td3_target_actions: mu {tuple(mu.shape)} against next_obs_act "
                         f"{tuple(next_obs_act.shape)}")
    B, A = mu.shape
    D = next_obs_act.shape[1] - A
    dev, f = mu.device, torch.float32
    if policy_noise != 0 and counter is None:
        raise ValueError("td3_target_actions: policy_noise != 0 needs the device counter")
    call("ocppo_td3_target_actions", _stream(dev), _check(mu, "mu", f), B, D, A,
         _td3_vec(action_scale, "action_scale", A, dev), _td3_vec(action_bias, "action_bias", A, dev),
         int(seed) & 0xFFFFFFFFFFFFFFFF, _opt(counter, "counter", torch.int64, dev, 1),
         float(policy_noise), float(noise_clip), float(low), float(high),
         _check(next_obs_act, "next_obs_act", f, dev, B * (D + A)))
    return next_obs_act


def td3_critic_loss_fwd_bwd(q1t, q2t, q1, q2, rewards, dones, gamma: float, dq1=None, dq2=None,
                            stats=None, y_out=None):
    """td3_continuous_action.py:248-255 from the four critic outputs [B] (or [B, 1]): (stats [4] =
    {qf1_loss, qf2_loss, mean q1, mean q2}, dq1, dq2 = d qf_loss / d q). q2t = q2 = None: the
    single critic of ddpg_continuous_action.py:218-221 (stats[1] = stats[3] = 0, dq2 None)."""
    B = q1.numel()
    dev, f = q1.device, torch.float32
    twin = q2 is not None
    if twin != (q2t is not None):
        raise ValueError("td3_critic_loss_fwd_bwd: q2 and its target come together")
    if dq1 is None:
        dq1 = torch.empty_like(q1)
    if twin and dq2 is None:
        dq2 = torch.empty_like(q2)
    if stats is None:
        stats = torch.empty(4, dtype=f, device=dev)
    call("ocppo_td3_critic_loss_fwd_bwd", _stream(dev), _check(q1t, "q1t", f, dev, B),
         _opt(q2t, "q2t", f, dev, B), _check(q1, "q1", f, dev, B), _opt(q2, "q2", f, dev, B),
         _check(rewards, "rewards", f, dev, B), _check(dones, "dones", f, dev, B), B, float(gamma),
         _check(dq1, "dq1", f, dev, B), _check(dq2, "dq2", f, dev, B) if twin else None,
         _check(stats, "stats", f, dev, 4), _opt(y_out, "y_out", f, dev, B))
    return stats, dq1, (dq2 if twin else None)


class _PolicyActions(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, obs_act, action_scale, action_bias):
        B, A = mu.shape
        D = obs_act.shape[1] - A
        dev, f = mu.device, torch.float32
        xa = torch.empty_like(obs_act)
        th = torch.empty_like(mu)
        call("ocppo_td3_policy_actions_fwd", _stream(dev), _check(mu, "mu", f), _check(
            obs_act, "obs_act", f, dev, B * (D + A)), B, D, A,
            _td3_vec(action_scale, "action_scale", A, dev),
            _td3_vec(action_bias, "action_bias", A, dev), xa.data_ptr(), th.data_ptr())
        ctx.save_for_backward(th, action_scale)
        ctx.D = D
        return xa

    @staticmethod
    def backward(ctx, dxa):
        th, scale = ctx.saved_tensors
        B, A = th.shape
        dev = th.device
        dxa = dxa.contiguous()
        dmu = torch.empty_like(th)
        call("ocppo_td3_policy_actions_bwd", _stream(dev),
             _check(dxa, "dxa", torch.float32, dev, B * (ctx.D + A)), th.data_ptr(), B, ctx.D, A,
             scale.data_ptr(), dmu.data_ptr())
        return dmu, None, None, None


def td3_policy_actions(mu, obs_act, action_scale, action_bias):
    """The critic's input of the actor loss (td3_continuous_action.py:263): a [B, D + A] copy of
    obs_act with its action columns replaced by tanh(mu) * scale + bias; differentiable in mu
    (d mu = (dxa[:, D:] * scale) * (1 - tanh^2), two launches in all)."""
    if mu.dim() != 2 or obs_act.dim() != 2 or obs_act.shape[0] != mu.shape[0] or \
            obs_act.shape[1] <= mu.shape[1] or not 1 <= mu.shape[1] <= GAUSS_MAX_ACTIONS:
        raise ValueError(f"td3_policy_actions: mu {tuple(mu.shape)} against obs_act "
                         f"{tuple(obs_act.shape)}")
    return _PolicyActions.apply(mu, obs_act, action_scale, action_bias)


POLYAK_MAX_PAIRS = 4


def polyak_(pairs, tau: float):
    """target = tau * param + (1 - tau) * target for every (flat parameter, flat target) pair, in
    place, one launch (td3_continuous_action.py:269-274): two rounded products and one rounded add
    per element, bitwise `target.copy_(tau * param + (1.0 - tau) * target)`."""
    pairs = list(pairs)
    n = len(pairs)
    if not 1 <= n <= POLYAK_MAX_PAIRS:
        raise ValueError(f"polyak_: {n} pairs, expected 1..{POLYAK_MAX_PAIRS}")
    dev = pairs[0][0].device
    ps, ts, ns = [], [], []
    for k, (p, t) in enumerate(pairs):
        if p.numel() != t.numel():
            raise ValueError(f"polyak_: pair {k}: {p.numel()} parameters, {t.numel()} targets")
        ps.append(_check(p, f"param[{k}]", torch.float32, dev))
        ts.append(_check(t, f"target[{k}]", torch.float32, dev))
        ns.append(p.numel())
    c = ctypes
    call("ocppo_polyak", _stream(dev), n, (c.c_void_p * n)(*ps), (c.c_void_p * n)(*ts),
         (c.c_int64 * n)(*ns), float(tau))


# ---------------------------------------------------------------------------------------------
# Continuous SAC (sac_continuous_action.py): acting, get_action on the heads' outputs, the
# entropy-regularised critic loss, the actor loss and the temperature step
# (csrc/ocppo_sac_cont.hip); the replay and the soft update are TD3's
# ---------------------------------------------------------------------------------------------
def csac_policy_draw(i: int) -> int:
    """The draw index of the policy's sample in iteration i of a policy step (:286)."""
    return 1 + 2 * int(i)


def csac_alpha_draw(i: int) -> int:
    """The draw index of the temperature's fresh sample in iteration i (:298)."""
    return 2 + 2 * int(i)


CSAC_TARGET_DRAW = 0  # the target's sample (:265)


def _csac_heads(mean, r, who: str):
    if mean.dim() != 2 or r.shape != mean.shape or not 1 <= mean.shape[1] <= GAUSS_MAX_ACTIONS:
        raise ValueError(f"{who}: mean {tuple(mean.shape)} against r {tuple(r.shape)} (A at most "
                         f"{GAUSS_MAX_ACTIONS})")
    return mean.shape


def csac_act(hidden, w_mean, b_mean, w_logstd, b_logstd, action_scale, action_bias, low, high,
             seed: int, step, learning_starts: int, actions_out=None, step_offset: int = 0):
    """sac_continuous_action.py:233-237 at global step t = step[0] + step_offset, from the actor's
    last hidden [E, H] (H a multiple of 64): t < learning_starts: uniform in [low, high) per
    dimension; otherwise tanh(mean + exp(log_std) * z) * scale + bias with both heads in
    td3.act_mu's summation order and log_std = -5 + 3.5 * (tanh(r) + 1). One launch; the branch is
    taken on the device. csac_noise returns z (and the uniform u)."""
    if hidden.dim() != 2 or w_mean.dim() != 2 or w_mean.shape[1] != hidden.shape[1] or \
            w_logstd.shape != w_mean.shape:
        raise ValueError(f"csac_act: hidden {tuple(hidden.shape)} against w_mean "
                         f"{tuple(w_mean.shape)}, w_logstd {tuple(w_logstd.shape)}")
    E, H = hidden.shape
    A = w_mean.shape[0]
    if not 1 <= A <= GAUSS_MAX_ACTIONS:
        raise ValueError(f"csac_act: A = {A} action dimensions, at most {GAUSS_MAX_ACTIONS}")
    if H % 64:
        raise ValueError(f"csac_act: hidden width {H} is not a multiple of 64")
    dev, f = hidden.device, torch.float32
    if actions_out is None:
        actions_out = torch.empty((E, A), dtype=f, device=dev)
    call("ocppo_csac_act", _stream(dev), _check(hidden, "hidden", f), E, H,
         _check(w_mean, "w_mean", f, dev, A * H), _check(b_mean, "b_mean", f, dev, A),
         _check(w_logstd, "w_logstd", f, dev, A * H), _check(b_logstd, "b_logstd", f, dev, A), A,
         _td3_vec(action_scale, "action_scale", A, dev), _td3_vec(action_bias, "action_bias", A, dev),
         _td3_vec(low, "low", A, dev), _td3_vec(high, "high", A, dev),
         int(seed) & 0xFFFFFFFFFFFFFFFF, _check(step, "step", torch.int64, dev, 1),
         int(step_offset), int(learning_starts), _check(actions_out, "actions", f, dev, E * A))
    return actions_out


def csac_noise(seed: int, counter, rows: int, A: int, draw: int | None = None, offset: int = 0,
               uniform: bool = False, out=None):
    """The [rows, A] draws of the continuous-SAC streams. draw None: the acting stream at global
    step counter[0] + offset (the standard normal z, or with `uniform` the random phase's u);
    draw >= 0: the update stream's z of that draw index (CSAC_TARGET_DRAW, csac_policy_draw(i),
    csac_alpha_draw(i)) at sample counter counter[0] + offset."""
    dev = counter.device
    if not 1 <= A <= GAUSS_MAX_ACTIONS:
        raise ValueError(f"csac_noise: A = {A}, expected 1..{GAUSS_MAX_ACTIONS}")
    if draw is not None and uniform:
        raise ValueError("csac_noise: the uniform draw belongs to the acting stream (draw None)")
    if out is None:
        out = torch.empty((rows, A), dtype=torch.float32, device=dev)
    mode = 2 if draw is not None else (1 if uniform else 0)
    call("ocppo_csac_noise", _stream(dev), int(seed) & 0xFFFFFFFFFFFFFFFF,
         _check(counter, "counter", torch.int64, dev, 1), int(offset), int(rows), A, mode,
         int(draw or 0), _check(out, "out", torch.float32, dev, rows * A))
    return out


def _csac_sample_fwd(mean, r, action_scale, action_bias, seed, counter, draw, obs_act, xa, saved,
                     z=None):
    B, A = mean.shape
    dev, f = mean.device, torch.float32
    D = xa.shape[1] - A if xa is not None else 1
    logp = torch.empty((B, 1), dtype=f, device=dev)
    n = B * A
    call("ocppo_csac_sample_fwd", _stream(dev), _check(mean, "mean", f, dev, n),
         _check(r, "r", f, dev, n), B, D, A, _td3_vec(action_scale, "action_scale", A, dev),
         _td3_vec(action_bias, "action_bias", A, dev), int(seed) & 0xFFFFFFFFFFFFFFFF,
         _opt(counter, "counter", torch.int64, dev, 1), int(draw), _opt(z, "z", f, dev, n),
         _opt(obs_act, "obs_act", f, dev, B * (D + A)), _opt(xa, "xa", f, dev, B * (D + A)),
         logp.data_ptr(), *(t.data_ptr() if t is not None else None for t in saved))
    return logp


class _CsacSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, r, obs_act, action_scale, action_bias, seed, counter, draw, z_in):
        B, A = mean.shape
        xa = torch.empty_like(obs_act)
        y, z, ls = (torch.empty_like(mean) for _ in range(3))
        logp = _csac_sample_fwd(mean, r, action_scale, action_bias, seed, counter, draw, obs_act,
                                xa, (y, z, ls), z_in)
        ctx.save_for_backward(mean, r, y, z, ls, action_scale)
        ctx.D = obs_act.shape[1] - A
        ctx.mark_non_differentiable(y, z, ls)
        return xa, logp, y, z, ls

    @staticmethod
    def backward(ctx, dxa, dlogp, *_):
        mean, r, y, z, ls, scale = ctx.saved_tensors
        B, A = y.shape
        dev, f = y.device, torch.float32
        dxa = torch.zeros((B, ctx.D + A), dtype=f, device=dev) if dxa is None else dxa.contiguous()
        dlogp = torch.zeros((B, 1), dtype=f, device=dev) if dlogp is None else dlogp.contiguous()
        dmean, dr = torch.empty_like(y), torch.empty_like(y)
        call("ocppo_csac_sample_bwd", _stream(dev), _check(dxa, "dxa", f, dev, B * (ctx.D + A)),
             _check(dlogp, "dlogp", f, dev, B), mean.data_ptr(), r.data_ptr(), y.data_ptr(), z.data_ptr(),
             ls.data_ptr(), B, ctx.D, A, scale.data_ptr(), dmean.data_ptr(), dr.data_ptr())
        return dmean, dr, None, None, None, None, None, None, None


def csac_sample(mean, r, obs_act, action_scale, action_bias, seed: int = 0, counter=None,
                draw: int = 0, aux: bool = False, z=None):
    """get_action (sac_continuous_action.py:138-150) on the heads' outputs mean, r [B, A] with
    the update stream's draw `draw` at sample counter counter[0]: (xa, log_prob [B, 1]), xa a
    [B, D + A] copy of obs_act with its action columns replaced by tanh(mean + exp(log_std) * z) *
    scale + bias. Differentiable in mean and r (two launches in all). aux: also (y, z, log_std).
    z [B, A]: the draws are these, not the stream's (then no counter is needed)."""
    _csac_heads(mean, r, "csac_sample")
    if z is None and counter is None:
        raise ValueError("csac_sample: the stream's draw needs the device counter")
    if obs_act.dim() != 2 or obs_act.shape[0] != mean.shape[0] or \
            obs_act.shape[1] <= mean.shape[1]:
        raise ValueError(f"csac_sample: mean {tuple(mean.shape)} against obs_act "
                         f"{tuple(obs_act.shape)}")
    xa, logp, y, z, ls = _CsacSample.apply(mean, r.contiguous(), obs_act, action_scale,
                                           action_bias, seed, counter, draw, z)
    return (xa, logp, y, z, ls) if aux else (xa, logp)


def csac_sample_forward(mean, r, action_scale, action_bias, seed: int = 0, counter=None,
                        draw: int = 0, xa=None, z=None):
    """The forward-only mode of csac_sample, one launch, no graph: log_prob [B, 1] of the draw;
    xa [B, D + A], if given, receives the action in its action columns (the target's
    next_obs_act: its observation columns stay). z: as csac_sample."""
    B, A = _csac_heads(mean, r, "csac_sample_forward")
    if z is None and counter is None:
        raise ValueError("csac_sample_forward: the stream's draw needs the device counter")
    if xa is not None and (xa.dim() != 2 or xa.shape[0] != B or xa.shape[1] <= A):
        raise ValueError(f"csac_sample_forward: mean {tuple(mean.shape)} against xa "
                         f"{tuple(xa.shape)}")
    return _csac_sample_fwd(mean, r, action_scale, action_bias, seed, counter, draw, None, xa,
                            (None, None, None), z)


def csac_critic_loss_fwd_bwd(q1t, q2t, q1, q2, rewards, dones, next_log_prob, alpha, gamma: float,
                             dq1=None, dq2=None, stats=None, y_out=None):
    """sac_continuous_action.py:264-275 from the four critic outputs and the next log-prob [B] (or
    [B, 1]) and the device scalar alpha: (stats [4] = {qf1_loss, qf2_loss, mean q1, mean q2}, dq1,
    dq2 = d qf_loss / d q); y = r + (1 - d) * gamma * (min(q1t, q2t) - alpha * next_log_prob)."""
    B = q1.numel()
    dev, f = q1.device, torch.float32
    if dq1 is None:
        dq1 = torch.empty_like(q1)
    if dq2 is None:
        dq2 = torch.empty_like(q2)
    if stats is None:
        stats = torch.empty(4, dtype=f, device=dev)
    call("ocppo_csac_critic_loss_fwd_bwd", _stream(dev), _check(q1t, "q1t", f, dev, B),
         _check(q2t, "q2t", f, dev, B), _check(q1, "q1", f, dev, B), _check(q2, "q2", f, dev, B),
         _check(rewards, "rewards", f, dev, B), _check(dones, "dones", f, dev, B),
         _check(next_log_prob, "next_log_prob", f, dev, B), _check(alpha, "alpha", f, dev, 1), B,
         float(gamma), _check(dq1, "dq1", f, dev, B), _check(dq2, "dq2", f, dev, B),
         _check(stats, "stats", f, dev, 4), _opt(y_out, "y_out", f, dev, B))
    return stats, dq1, dq2


def csac_actor_loss_fwd_bwd(q1_pi, q2_pi, log_prob, alpha, dq1=None, dq2=None, dlogp=None,
                            loss=None):
    """sac_continuous_action.py:287-290: (loss [1] = mean(alpha * log_prob - min(q1_pi, q2_pi)),
    dq1, dq2, dlogp), the min's gradient routed as torch.min's backward (ties: half each)."""
    B = q1_pi.numel()
    dev, f = q1_pi.device, torch.float32
    if dq1 is None:
        dq1 = torch.empty_like(q1_pi)
    if dq2 is None:
        dq2 = torch.empty_like(q2_pi)
    if dlogp is None:
        dlogp = torch.empty_like(log_prob)
    if loss is None:
        loss = torch.empty(1, dtype=f, device=dev)
    call("ocppo_csac_actor_loss_fwd_bwd", _stream(dev), _check(q1_pi, "q1_pi", f, dev, B),
         _check(q2_pi, "q2_pi", f, dev, B), _check(log_prob, "log_prob", f, dev, B),
         _check(alpha, "alpha", f, dev, 1), B, _check(dq1, "dq1", f, dev, B),
         _check(dq2, "dq2", f, dev, B), _check(dlogp, "dlogp", f, dev, B),
         _check(loss, "loss", f, dev, 1))
    return loss, dq1, dq2, dlogp


def csac_alpha_step(log_prob, temp: SacTemperature, loss=None):
    """sac_continuous_action.py:296-304 on the fresh draw's log_prob [B]: loss [1] =
    mean(-exp(log_alpha) * (log_prob + target_entropy)), log_alpha's Adam step and alpha =
    exp(log_alpha) on temp's buffers, one launch. temp.autotune only."""
    if not temp.autotune:
        raise ValueError("csac_alpha_step: the temperature is a constant (autotune off)")
    B = log_prob.numel()
    dev, f = log_prob.device, torch.float32
    if loss is None:
        loss = torch.empty(1, dtype=f, device=dev)
    call("ocppo_csac_alpha_step", _stream(dev), _check(log_prob, "log_prob", f, dev, B), B,
         _check(temp.alpha, "alpha", f, dev, 1), _check(temp.log_alpha, "log_alpha", f, dev, 1),
         temp.target_entropy, _check(temp.exp_avg, "exp_avg", f, dev, 1),
         _check(temp.exp_avg_sq, "exp_avg_sq", f, dev, 1),
         _check(temp.step, "adam_step", torch.int64, dev, 1), temp.lr, temp.betas[0],
         temp.betas[1], temp.eps, _check(loss, "loss", f, dev, 1))
    return loss


# ---------------------------------------------------------------------------------------------
# MaDi's masker (architectures/madi.py MaskerNet; ppo_atari_madi.py:441, :502): the gather, x / 255,
# the three padded convolutions, the sigmoid and the multiply as one launch, and the six parameter
# gradients with the activations recomputed per tile (csrc/ocppo_madi.hip)
# ---------------------------------------------------------------------------------------------
MADI_FILTERS = (16, 32)
# Calls of more stacks than this run the torch modules: 512 stacks of 4 x 84 x 84 is the largest
# call of either kernel that has run to its end on hardware
MADI_MAX_STACKS = 512
# A differentiated call (the update) on the kernels. As single launches at 320 stacks (the
# script's 10 envs) the fused forward + backward takes 21.6 ms against 16.3 ms for the torch
# modules with MIOpen free to choose; in the learner, whose torch_deterministic default restricts
# MIOpen, the update on the torch modules runs at 310 env steps/s and on the kernels at 3,072
# (tools/exp_madi.py)
MADI_FUSED_UPDATE = True


def madi_ok(src, weights, num_layers: int = 3, padding_mode: str = "zeros", stacks=None,
            backward: bool = False) -> bool:
    """The fused masker applies to a call of `stacks` stacks (None: every row of src): three
    layers, 16 or 32 filters, zero padding, u8 or f32 square frame stacks [rows, W, H, H] and the
    six masker tensors (w1, b1, w2, b2, w3, b3), all on the GPU, at most MADI_MAX_STACKS stacks;
    backward: the call is differentiated (MADI_FUSED_UPDATE). Anything else runs the torch
    modules."""
    if num_layers != 3 or padding_mode != "zeros" or len(weights) != 6:
        return False
    if not isinstance(src, torch.Tensor) or src.device.type != "cuda" or src.dim() != 4 or \
            src.shape[2] != src.shape[3] or src.dtype not in (torch.uint8, torch.float32) or \
            min(src.shape) < 1:
        return False
    w1, b1, w2, b2, w3, b3 = weights
    F = w1.shape[0]
    if F not in MADI_FILTERS:
        return False
    shapes = ((F, 1, 3, 3), (F,), (F, F, 3, 3), (F,), (1, F, 3, 3), (1,))
    if any(t.device != src.device or t.dtype != torch.float32 or tuple(t.shape) != s
           for t, s in zip(weights, shapes)):
        return False
    n = src.shape[0] if stacks is None else stacks
    return n <= MADI_MAX_STACKS and (MADI_FUSED_UPDATE or not backward)


def _madi_args(src, idx, weights, who):
    if src.dim() != 4 or src.shape[2] != src.shape[3] or src.dtype not in (torch.uint8,
                                                                            torch.float32):
        raise ValueError(f"{who}: src must be u8 or f32 [rows, W, H, H], got "
                         f"{tuple(src.shape)} {src.dtype}")
    dev = src.device
    rows, W, H, _ = src.shape
    w1 = weights[0]
    F = w1.shape[0]
    if F not in MADI_FILTERS:
        raise ValueError(f"{who}: {F} filters (supported: {MADI_FILTERS})")
    shapes = ((F, 1, 3, 3), (F,), (F, F, 3, 3), (F,), (1, F, 3, 3), (1,))
    ptrs = []
    for t, s, n in zip(weights, shapes, ("w1", "b1", "w2", "b2", "w3", "b3")):
        if tuple(t.shape) != s:
            raise ValueError(f"{who}: {n} must be {s}, got {tuple(t.shape)}")
        ptrs.append(_check(t, n, torch.float32, dev))
    B = rows if idx is None else idx.numel()
    if min(rows, W, H, B) < 1:
        raise ValueError(f"{who}: empty input")
    head = (_stream(dev), _check(src, "src", None, dev), _DTYPE_CODE[src.dtype],
            _opt(idx, "idx", torch.int64, dev), rows, B, W, H, F, *ptrs)
    return head, dev, B, W, H, F


def _madi_layout(t, B, W, H, dev, name):
    """channels_last flag of a masked-stack buffer [B, W, H, H] f32 (contiguous or
    channels_last)."""
    if t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (B, W, H, H):
        raise ValueError(f"{name}: expected f32 {(B, W, H, H)} on {dev}")
    if t.is_contiguous():
        return 0
    if t.is_contiguous(memory_format=torch.channels_last):
        return 1
    raise ValueError(f"{name}: must be contiguous or channels_last")


def madi_mask(src, idx, weights, out=None, channels_last: bool = False):
    """MaskerNet.forward of the stacks src[idx] (idx None: every row in order) in one launch:
    out [B, W, H, H] f32 = x * sigmoid(conv3(relu(conv2(relu(conv1(x / 255)))))), every frame on
    its own. weights: (w1, b1, w2, b2, w3, b3). out: contiguous or channels_last (made in the
    format `channels_last` names when None)."""
    head, dev, B, W, H, F = _madi_args(src, idx, weights, "madi_mask")
    if out is None:
        out = torch.empty((B, W, H, H), dtype=torch.float32, device=dev,
                          memory_format=torch.channels_last if channels_last
                          else torch.contiguous_format)
    call("ocppo_madi_mask_fwd", *head, _madi_layout(out, B, W, H, dev, "out"), out.data_ptr())
    return out


def madi_workspace(F: int, device):
    """The backward's partial rows: ocppo_madi_workspace_bytes(F), the same for any number of
    frames."""
    nb = int(_lib.LIB.ocppo_madi_workspace_bytes(F))
    if nb == 0:
        raise ValueError(f"madi_workspace: {F} filters (supported: {MADI_FILTERS})")
    return torch.empty(nb // 4, dtype=torch.float32, device=device)


def madi_mask_bwd(src, idx, weights, g, grads=None, workspace=None):
    """The six parameter gradients of madi_mask for g = dL/d(out) (out's layout). grads: six
    contiguous f32 tensors of the weights' shapes to write (made when None). Deterministic: two
    calls on the same inputs are bitwise equal."""
    head, dev, B, W, H, F = _madi_args(src, idx, weights, "madi_mask_bwd")
    if grads is None:
        grads = tuple(torch.empty_like(w, memory_format=torch.contiguous_format) for w in weights)
    if workspace is None:
        workspace = _persistent("madi_mask_bwd", dev, F, lambda: madi_workspace(F, dev))
    gp = [_check(d, f"grads[{i}]", torch.float32, dev, w.numel())
          for i, (d, w) in enumerate(zip(grads, weights))]
    call("ocppo_madi_mask_bwd", *head, _madi_layout(g, B, W, H, dev, "g"), g.data_ptr(), *gp,
         _check(workspace, "workspace", torch.float32, dev), workspace.numel() * 4)
    return grads
