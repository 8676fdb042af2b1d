"""The log-likelihood of (input sequence, profile) pairs as a differentiable function of the profiles, for PyTorch: a CTC-style loss
with a transducer (an error or channel model) between the truth and the frames (docs/profile_tapes.md, "Row posteriors").

The gradient of a pair's log-likelihood in its profile is the pair's row posteriors, so forward is one row_posteriors() call and
backward multiplies what it kept.  The machine's weights are constants here; their gradient is the posterior counts
(capi.DeviceProfilePairs.counts).
"""
from __future__ import annotations

import numpy as np
import torch


def _row_posteriors(machine_or_dm, inputs, P, rowOff, envs, backend):
    """(post[sumRows, C], loglike[nPairs]) in numpy, on the device or by the numpy yardstick."""
    n = len(rowOff) - 1
    profiles = [P[rowOff[k]:rowOff[k + 1]] for k in range(n)]
    if backend == "numpy":
        from .profile import PairProfileDP
        em = getattr(machine_or_dm, "em", machine_or_dm)
        dp = PairProfileDP(em)
        post = np.zeros(P.shape, np.float64)
        ll = np.empty(n, np.float64)
        for k in range(n):
            post[rowOff[k]:rowOff[k + 1]], ll[k] = dp.rowPosteriors(inputs[k], profiles[k], env=None if envs is None else envs[k])
        return post, ll
    if backend != "device":
        raise ValueError('backend is "device" or "numpy"')
    from . import capi
    own = not isinstance(machine_or_dm, capi.DeviceMachine)
    dm = capi.DeviceMachine(machine_or_dm) if own else machine_or_dm
    pairs = capi.DeviceProfilePairs(dm, inputs, profiles)
    try:
        if envs is not None:
            pairs.set_envelopes(envs)
        return pairs.row_posteriors()
    finally:
        pairs.close()
        if own:
            dm.close()


class _PairProfileLoglike(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logP, machine_or_dm, inputs, rowOff, envs, backend):
        P = np.ascontiguousarray(logP.detach().cpu().numpy(), np.float64)
        post, ll = _row_posteriors(machine_or_dm, inputs, P, rowOff, envs, backend)
        ctx.rowOff = rowOff
        ctx.save_for_backward(torch.from_numpy(post).to(logP.device))
        return torch.from_numpy(ll).to(logP.device)

    @staticmethod
    def backward(ctx, grad_out):
        post, = ctx.saved_tensors
        rows = torch.as_tensor(np.diff(ctx.rowOff), device=post.device)
        return torch.repeat_interleave(grad_out.to(post.dtype), rows).unsqueeze(1) * post, None, None, None, None, None


def pair_profile_loglike(machine_or_dm, inputs, logP, rowOff, envs=None, backend="device"):
    """tensor[nPairs] of log-likelihoods: pair k is the token sequence ``inputs[k]`` (1..nInTok) against the rows
    rowOff[k]..rowOff[k + 1] of ``logP``, a float64 [sumRows, nOutTok + 1] tensor of log weights with column 0 the blank.
    Differentiable in ``logP``: the gradient is grad_out[k] times the row posteriors of pair k, zeros for a pair that scores -inf
    (like zero_infinity of a CTC loss).  ``machine_or_dm``: an EvaluatedMachine or a capi.DeviceMachine (kept open for the
    caller).  ``envs``: per pair None, a seqpair.Envelope or (inStart, inEnd).  ``backend``: "device" (one
    capi.DeviceProfilePairs.row_posteriors() call) or "numpy" (profile.PairProfileDP.rowPosteriors, no GPU needed).

    Tensors of any device go through host memory (``.detach().cpu().numpy()``) and the results come back to the tensor's device;
    a zero-copy entry that takes device pointers is out of scope here."""
    if logP.dtype != torch.float64 or logP.dim() != 2:
        raise ValueError("logP is a float64 [sumRows, nOutTok + 1] tensor")
    rowOff = np.asarray(rowOff, np.int64).reshape(-1)
    if len(rowOff) != len(inputs) + 1 or rowOff[0] != 0 or rowOff[-1] != logP.shape[0] or (np.diff(rowOff) < 0).any():
        raise ValueError("rowOff has one entry per pair and one more, from 0 up to the rows of logP")
    if envs is not None and len(envs) != len(inputs):
        raise ValueError("one envelope (or None) per pair, please")
    inputs = [np.asarray(x, np.int64).reshape(-1) for x in inputs]
    return _PairProfileLoglike.apply(logP, machine_or_dm, inputs, rowOff, envs, backend)
