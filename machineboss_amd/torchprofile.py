"""The log-likelihood of (input sequence, profile) pairs as a differentiable function of the profiles, for PyTorch: a CTC-style loss
with a transducer (an error or channel model) between the truth and the frames (docs/profile_tapes.md, "Row posteriors"); and of
(input profile, output profile) pairs as a differentiable function of both (two_profile_loglike); and of one-tape profiles scored
by a generator (profile_loglike), which with CTC-merged profiles is the CTC loss proper, constrained to the generator's language.

The gradient of a pair's log-likelihood in its profile is the pair's row posteriors, so forward is one row_posteriors() call and
backward multiplies what it kept.  The machine's weights are constants here; their gradient is the posterior counts
(capi.DeviceProfilePairs.counts).
"""
from __future__ import annotations

import numpy as np
import torch


def _row_posteriors(machine_or_dm, inputs, P, rowOff, envs, backend, colTok=None):
    """(post[sumRows, width], loglike[nPairs]) in numpy, on the device or by the numpy yardstick; colTok: CTC-merged profiles."""
    n = len(rowOff) - 1
    profiles = [P[rowOff[k]:rowOff[k + 1]] for k in range(n)]
    if backend == "numpy":
        from .profile import PairMergedProfileDP, PairProfileDP
        em = getattr(machine_or_dm, "em", machine_or_dm)
        dp = PairProfileDP(em) if colTok is None else PairMergedProfileDP(em, colTok)
        post = np.zeros(P.shape, np.float64)
        ll = np.empty(n, np.float64)
        for k in range(n):
            if colTok is None:
                post[rowOff[k]:rowOff[k + 1]], ll[k] = dp.rowPosteriors(inputs[k], profiles[k], env=None if envs is None else envs[k])
            elif envs is None or envs[k] is None:
                post[rowOff[k]:rowOff[k + 1]], ll[k] = dp.rowPosteriors(inputs[k], profiles[k])
            else:
                post[rowOff[k]:rowOff[k + 1]], ll[k] = dp.rowPosteriors(inputs[k], profiles[k], env=envs[k])
        return post, ll
    if backend != "device":
        raise ValueError('backend is "device" or "numpy"')
    from . import capi
    own = not isinstance(machine_or_dm, capi.DeviceMachine)
    dm = capi.DeviceMachine(machine_or_dm) if own else machine_or_dm
    pairs = None
    try:
        pairs = capi.DeviceProfilePairs(dm, inputs, profiles, colTok)
        if envs is not None and colTok is None:
            pairs.set_envelopes(envs)
        elif envs is not None:
            pairs.set_merged_envelopes(envs)
        return pairs.row_posteriors() if colTok is None else pairs.merged_row_posteriors()
    finally:
        if pairs is not None:
            pairs.close()
        if own:
            dm.close()


class _PairProfileLoglike(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logP, machine_or_dm, inputs, rowOff, envs, backend, colTok=None):
        P = np.ascontiguousarray(logP.detach().cpu().numpy(), np.float64)
        post, ll = _row_posteriors(machine_or_dm, inputs, P, rowOff, envs, backend, colTok)
        ctx.rowOff = rowOff
        ctx.save_for_backward(torch.from_numpy(post).to(logP.device))
        return torch.from_numpy(ll).to(logP.device)

    @staticmethod
    def backward(ctx, grad_out):
        post, = ctx.saved_tensors
        rows = torch.as_tensor(np.diff(ctx.rowOff), device=post.device)
        return torch.repeat_interleave(grad_out.to(post.dtype), rows).unsqueeze(1) * post, None, None, None, None, None, None


def pair_profile_loglike(machine_or_dm, inputs, logP, rowOff, envs=None, backend="device", colTok=None):
    """tensor[nPairs] of log-likelihoods: pair k is the token sequence ``inputs[k]`` (1..nInTok) against the rows
    rowOff[k]..rowOff[k + 1] of ``logP``, a float64 [sumRows, nOutTok + 1] tensor of log weights with column 0 the blank.
    Differentiable in ``logP``: the gradient is grad_out[k] times the row posteriors of pair k, zeros for a pair that scores -inf
    (like zero_infinity of a CTC loss).  ``machine_or_dm``: an EvaluatedMachine or a capi.DeviceMachine (kept open for the
    caller).  ``envs``: per pair None, a seqpair.Envelope or (inStart, inEnd).  ``backend``: "device" (one
    capi.DeviceProfilePairs.row_posteriors() call) or "numpy" (profile.PairProfileDP.rowPosteriors, no GPU needed).

    With ``colTok`` the profiles are CTC-merged frames: ``logP`` is [sumRows, nCols + 1], column c a frame's log weight of the
    output token colTok[c - 1], repeats collapse and a blank separates equal symbols (docs/profile_tapes.md, "Row posteriors of
    pairs against a merged profile").  Both backends take the merged route (capi.DeviceProfilePairs.merged_row_posteriors,
    profile.PairMergedProfileDP.rowPosteriors); with a one-state echo transducer the result is -ctc_loss(logP, x) per pair.
    Envelopes take plain profiles here; merged_pair_profile_loglike takes both.

    Tensors of any device go through host memory (``.detach().cpu().numpy()``) and the results come back to the tensor's device;
    a zero-copy entry that takes device pointers is out of scope here."""
    if logP.dtype != torch.float64 or logP.dim() != 2:
        raise ValueError("logP is a float64 [sumRows, nOutTok + 1] tensor")
    rowOff = np.asarray(rowOff, np.int64).reshape(-1)
    if len(rowOff) != len(inputs) + 1 or rowOff[0] != 0 or rowOff[-1] != logP.shape[0] or (np.diff(rowOff) < 0).any():
        raise ValueError("rowOff has one entry per pair and one more, from 0 up to the rows of logP")
    if envs is not None and len(envs) != len(inputs):
        raise ValueError("one envelope (or None) per pair, please")
    if colTok is not None:
        if envs is not None:
            raise ValueError("envelopes take plain profiles")
        colTok = np.asarray(colTok, np.int64).reshape(-1)
        if logP.shape[1] != len(colTok) + 1:
            raise ValueError("merged profiles: logP has one column per entry of colTok and the blank in front")
    inputs = [np.asarray(x, np.int64).reshape(-1) for x in inputs]
    return _PairProfileLoglike.apply(logP, machine_or_dm, inputs, rowOff, envs, backend, colTok)


def merged_pair_profile_loglike(machine_or_dm, inputs, logP, rowOff, colTok, envs=None, backend="device"):
    """pair_profile_loglike against CTC-merged frames, with envelopes: tensor[nPairs] of log-likelihoods, pair k the token sequence
    ``inputs[k]`` against the rows rowOff[k]..rowOff[k + 1] of ``logP``, a float64 [sumRows, nCols + 1] tensor with column 0 the blank
    and column c a frame's log weight of the output token colTok[c - 1].  ``envs``: per pair None, a seqpair.Envelope or (inStart,
    inEnd); a pair under one is summed over the alignments inside it alone (docs/profile_tapes.md, "Pairs against a merged profile
    under an envelope"), so its value is never above the unbanded one.  Differentiable in ``logP``: the gradient is grad_out[k] times
    the merged row posteriors of pair k under its envelope, zeros for a pair that scores -inf.  ``backend``: "device"
    (capi.DeviceProfilePairs.set_merged_envelopes, merged_row_posteriors) or "numpy" (profile.PairMergedProfileDP.rowPosteriors)."""
    if logP.dtype != torch.float64 or logP.dim() != 2:
        raise ValueError("logP is a float64 [sumRows, nCols + 1] tensor")
    rowOff = np.asarray(rowOff, np.int64).reshape(-1)
    if len(rowOff) != len(inputs) + 1 or rowOff[0] != 0 or rowOff[-1] != logP.shape[0] or (np.diff(rowOff) < 0).any():
        raise ValueError("rowOff has one entry per pair and one more, from 0 up to the rows of logP")
    if envs is not None and len(envs) != len(inputs):
        raise ValueError("one envelope (or None) per pair, please")
    colTok = np.asarray(colTok, np.int64).reshape(-1)
    if logP.shape[1] != len(colTok) + 1:
        raise ValueError("merged profiles: logP has one column per entry of colTok and the blank in front")
    inputs = [np.asarray(x, np.int64).reshape(-1) for x in inputs]
    return _PairProfileLoglike.apply(logP, machine_or_dm, inputs, rowOff, envs, backend, colTok)


def _two_row_posteriors(machine_or_dm, A, inOff, B, rowOff, wantA, wantB, envs, backend):
    """(postA[sumK, CA] or None, postB[sumRows, C] or None, loglike[nPairs]) in numpy, on the device or by the numpy yardstick."""
    n = len(rowOff) - 1
    As = [A[inOff[k]:inOff[k + 1]] for k in range(n)]
    Bs = [B[rowOff[k]:rowOff[k + 1]] for k in range(n)]
    if backend == "numpy":
        from .profile import TwoProfileDP
        em = getattr(machine_or_dm, "em", machine_or_dm)
        dp = TwoProfileDP(em)
        postA, postB = np.zeros(A.shape, np.float64), np.zeros(B.shape, np.float64)
        ll = np.empty(n, np.float64)
        for k in range(n):
            postA[inOff[k]:inOff[k + 1]], postB[rowOff[k]:rowOff[k + 1]], ll[k] = dp.rowPosteriors(As[k], Bs[k], env=None if envs is None else envs[k])
        return (postA if wantA else None), (postB if wantB else None), ll
    if backend != "device":
        raise ValueError('backend is "device" or "numpy"')
    from . import capi
    own = not isinstance(machine_or_dm, capi.DeviceMachine)
    dm = capi.DeviceMachine(machine_or_dm) if own else machine_or_dm
    twos = None
    try:
        twos = capi.DeviceProfileTwos(dm, As, Bs, envs=envs)
        return twos.row_posteriors(inputs=wantA, outputs=wantB)
    finally:
        if twos is not None:
            twos.close()
        if own:
            dm.close()


class _TwoProfileLoglike(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logA, logB, machine_or_dm, inOff, rowOff, envs, backend):
        A = np.ascontiguousarray(logA.detach().cpu().numpy(), np.float64)
        B = np.ascontiguousarray(logB.detach().cpu().numpy(), np.float64)
        wantA, wantB = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        postA, postB, ll = _two_row_posteriors(machine_or_dm, A, inOff, B, rowOff, wantA, wantB, envs, backend)
        ctx.inOff, ctx.rowOff = inOff, rowOff
        ctx.save_for_backward(None if postA is None else torch.from_numpy(postA).to(logA.device),
                              None if postB is None else torch.from_numpy(postB).to(logB.device))
        return torch.from_numpy(ll).to(logB.device)

    @staticmethod
    def backward(ctx, grad_out):
        def grad(post, off):
            if post is None:
                return None
            rows = torch.as_tensor(np.diff(off), device=post.device)
            return torch.repeat_interleave(grad_out.to(device=post.device, dtype=post.dtype), rows).unsqueeze(1) * post
        postA, postB = ctx.saved_tensors
        return grad(postA, ctx.inOff), grad(postB, ctx.rowOff), None, None, None, None, None


def two_profile_loglike(machine_or_dm, logA, inOff, logB, rowOff, envs=None, backend="device"):
    """tensor[nPairs] of log-likelihoods: pair k is the rows inOff[k]..inOff[k + 1] of ``logA``, a float64 [sumK, nInTok + 1] tensor
    of log weights on the input tape, against the rows rowOff[k]..rowOff[k + 1] of ``logB``, a float64 [sumRows, nOutTok + 1] tensor
    on the output tape; column 0 of either is its blank (docs/profile_tapes.md, "Row posteriors of pairs of profiles").
    Differentiable in both tables: the gradient is grad_out[k] times the row posteriors of pair k on that tape, zeros for a pair
    that scores -inf, computed only for the tables that require one.  ``machine_or_dm``: an EvaluatedMachine or a
    capi.DeviceMachine (kept open for the caller).  ``envs``: per pair None, a seqpair.Envelope or (inStart, inEnd) over the input
    rows per output row (docs/profile_tapes.md, "Pairs of profiles under an envelope"); the posteriors are then summed over the
    envelope cells.  ``backend``: "device" (one capi.DeviceProfileTwos.row_posteriors() call) or
    "numpy" (profile.TwoProfileDP.rowPosteriors, no GPU needed).  Tensors go through host memory, as pair_profile_loglike's do."""
    if logA.dtype != torch.float64 or logA.dim() != 2:
        raise ValueError("logA is a float64 [sumK, nInTok + 1] tensor")
    if logB.dtype != torch.float64 or logB.dim() != 2:
        raise ValueError("logB is a float64 [sumRows, nOutTok + 1] tensor")
    inOff = np.asarray(inOff, np.int64).reshape(-1)
    rowOff = np.asarray(rowOff, np.int64).reshape(-1)
    if len(inOff) < 1 or inOff[0] != 0 or inOff[-1] != logA.shape[0] or (np.diff(inOff) < 0).any():
        raise ValueError("inOff has one entry per pair and one more, from 0 up to the rows of logA")
    if len(rowOff) != len(inOff) or rowOff[0] != 0 or rowOff[-1] != logB.shape[0] or (np.diff(rowOff) < 0).any():
        raise ValueError("rowOff has one entry per pair and one more, from 0 up to the rows of logB")
    if envs is not None and len(envs) != len(inOff) - 1:
        raise ValueError("one envelope (or None) per pair, please")
    return _TwoProfileLoglike.apply(logA, logB, machine_or_dm, inOff, rowOff, envs, backend)


def _two_merged_row_posteriors(machine_or_dm, A, inOff, B, rowOff, colTok, wantA, wantB, backend, envs=None):
    """_two_row_posteriors against CTC-merged output rows: postB is [sumRows, nCols + 1]."""
    n = len(rowOff) - 1
    As = [A[inOff[k]:inOff[k + 1]] for k in range(n)]
    Bs = [B[rowOff[k]:rowOff[k + 1]] for k in range(n)]
    if backend == "numpy":
        from .profile import TwoMergedProfileDP
        em = getattr(machine_or_dm, "em", machine_or_dm)
        dp = TwoMergedProfileDP(em, colTok)
        postA, postB = np.zeros(A.shape, np.float64), np.zeros(B.shape, np.float64)
        ll = np.empty(n, np.float64)
        for k in range(n):
            postA[inOff[k]:inOff[k + 1]], postB[rowOff[k]:rowOff[k + 1]], ll[k] = (
                dp.mergedRowPosteriors(As[k], Bs[k]) if envs is None or envs[k] is None else dp.mergedRowPosteriors(As[k], Bs[k], env=envs[k]))
        return (postA if wantA else None), (postB if wantB else None), ll
    if backend != "device":
        raise ValueError('backend is "device" or "numpy"')
    from . import capi
    own = not isinstance(machine_or_dm, capi.DeviceMachine)
    dm = capi.DeviceMachine(machine_or_dm) if own else machine_or_dm
    twos = None
    try:
        twos = capi.DeviceProfileTwos(dm, As, Bs, colTok=colTok, mergedEnvs=envs)
        return twos.merged_row_posteriors(inputs=wantA, outputs=wantB)
    finally:
        if twos is not None:
            twos.close()
        if own:
            dm.close()


class _TwoMergedProfileLoglike(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logA, logB, machine_or_dm, inOff, rowOff, colTok, backend, envs):
        A = np.ascontiguousarray(logA.detach().cpu().numpy(), np.float64)
        B = np.ascontiguousarray(logB.detach().cpu().numpy(), np.float64)
        wantA, wantB = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        postA, postB, ll = _two_merged_row_posteriors(machine_or_dm, A, inOff, B, rowOff, colTok, wantA, wantB, backend, envs)
        ctx.inOff, ctx.rowOff = inOff, rowOff
        ctx.save_for_backward(None if postA is None else torch.from_numpy(postA).to(logA.device),
                              None if postB is None else torch.from_numpy(postB).to(logB.device))
        return torch.from_numpy(ll).to(logB.device)

    @staticmethod
    def backward(ctx, grad_out):      # (two tables, six constants)
        return _TwoProfileLoglike.backward(ctx, grad_out) + (None,)


def merged_two_profile_loglike(machine_or_dm, logA, inOff, logB, rowOff, colTok, envs=None, backend="device"):
    """two_profile_loglike against CTC-merged frames on the output tape: tensor[nPairs] of log-likelihoods, pair k the rows
    inOff[k]..inOff[k + 1] of ``logA``, a float64 [sumK, nInTok + 1] tensor (column 0 the input blank), against the rows
    rowOff[k]..rowOff[k + 1] of ``logB``, a float64 [sumRows, nCols + 1] tensor with column 0 the blank and column c a frame's log
    weight of the output token colTok[c - 1]; repeats collapse and a blank separates equal symbols (docs/profile_tapes.md, "Row
    posteriors of pairs of profiles against a merged profile").  Differentiable in both tables: the gradient is grad_out[k] times
    the merged row posteriors of pair k on that tape, zeros for a pair that scores -inf, computed only for the tables that require
    one.  With a one-hot ``logA`` and a one-state echo transducer the result is -ctc_loss(logB, x) per pair.  ``machine_or_dm``: an
    EvaluatedMachine or a capi.DeviceMachine (kept open for the caller).  ``envs``: per pair None, a seqpair.Envelope or (inStart,
    inEnd) over the input rows per output row (docs/profile_tapes.md, "Pairs of profiles against a merged profile under an
    envelope"); the likelihood and the posteriors are then summed over the envelope cells.  ``backend``: "device" (one
    capi.DeviceProfileTwos.merged_row_posteriors() call) or "numpy" (profile.TwoMergedProfileDP.mergedRowPosteriors, no GPU
    needed).  Tensors go through host memory, as pair_profile_loglike's do."""
    if logA.dtype != torch.float64 or logA.dim() != 2:
        raise ValueError("logA is a float64 [sumK, nInTok + 1] tensor")
    if logB.dtype != torch.float64 or logB.dim() != 2:
        raise ValueError("logB is a float64 [sumRows, nCols + 1] tensor")
    inOff = np.asarray(inOff, np.int64).reshape(-1)
    rowOff = np.asarray(rowOff, np.int64).reshape(-1)
    if len(inOff) < 1 or inOff[0] != 0 or inOff[-1] != logA.shape[0] or (np.diff(inOff) < 0).any():
        raise ValueError("inOff has one entry per pair and one more, from 0 up to the rows of logA")
    if len(rowOff) != len(inOff) or rowOff[0] != 0 or rowOff[-1] != logB.shape[0] or (np.diff(rowOff) < 0).any():
        raise ValueError("rowOff has one entry per pair and one more, from 0 up to the rows of logB")
    colTok = np.asarray(colTok, np.int64).reshape(-1)
    if logB.shape[1] != len(colTok) + 1:
        raise ValueError("merged profiles: logB has one column per entry of colTok and the blank in front")
    if envs is not None and len(envs) != len(inOff) - 1:
        raise ValueError("one envelope (or None) per pair, please")
    return _TwoMergedProfileLoglike.apply(logA, logB, machine_or_dm, inOff, rowOff, colTok, backend, envs)


def _one_row_posteriors(machine_or_dm, P, rowOff, colTok, backend):
    """(post[sumRows, width], loglike[nProfiles]) in numpy, on the device or by the numpy yardstick."""
    n = len(rowOff) - 1
    profiles = [P[rowOff[k]:rowOff[k + 1]] for k in range(n)]
    if backend == "numpy":
        from .profile import MergedProfileDP, ProfileDP
        em = getattr(machine_or_dm, "em", machine_or_dm)
        dp = ProfileDP(em) if colTok is None else MergedProfileDP(em, colTok)
        post = np.zeros(P.shape, np.float64)
        ll = np.empty(n, np.float64)
        for k in range(n):
            post[rowOff[k]:rowOff[k + 1]], ll[k] = dp.rowPosteriors(profiles[k])
        return post, ll
    if backend != "device":
        raise ValueError('backend is "device" or "numpy"')
    from . import capi
    own = not isinstance(machine_or_dm, capi.DeviceMachine)
    dm = capi.DeviceMachine(machine_or_dm) if own else machine_or_dm
    prof = None
    try:
        prof = capi.DeviceProfiles(dm, profiles, colTok)
        return prof.row_posteriors()
    finally:
        if prof is not None:
            prof.close()
        if own:
            dm.close()


class _ProfileLoglike(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logP, machine_or_dm, rowOff, colTok, backend):
        P = np.ascontiguousarray(logP.detach().cpu().numpy(), np.float64)
        post, ll = _one_row_posteriors(machine_or_dm, P, rowOff, colTok, backend)
        ctx.rowOff = rowOff
        ctx.save_for_backward(torch.from_numpy(post).to(logP.device))
        return torch.from_numpy(ll).to(logP.device)

    @staticmethod
    def backward(ctx, grad_out):
        post, = ctx.saved_tensors
        rows = torch.as_tensor(np.diff(ctx.rowOff), device=post.device)
        return torch.repeat_interleave(grad_out.to(post.dtype), rows).unsqueeze(1) * post, None, None, None, None


def profile_loglike(machine_or_dm, logP, rowOff, colTok=None, backend="device"):
    """tensor[nProfiles] of log-likelihoods of a machine with an empty input alphabet (a generator) against one-tape profiles:
    profile k is the rows rowOff[k]..rowOff[k + 1] of ``logP``, a float64 [sumRows, nOutTok + 1] tensor of log weights with column 0
    the blank; with ``colTok`` the profiles are CTC-merged and logP is [sumRows, nCols + 1], column c a frame's log weight of the
    output token colTok[c - 1] (docs/profile_tapes.md, "Row posteriors of one-tape profiles").  With algebra.generator(y) as the
    machine and merged profiles the result is -ctc_loss(logP, y, reduction="sum") per profile; with a lexicon, a language model
    or a profile HMM it is the CTC likelihood of that generator's language.  Differentiable in ``logP``: the gradient is
    grad_out[k] times the row posteriors of profile k, zeros for a profile that scores -inf (like zero_infinity of a CTC loss).
    ``machine_or_dm``: an EvaluatedMachine or a capi.DeviceMachine (kept open for the caller).  ``backend``: "device" (one
    capi.DeviceProfiles.row_posteriors() call) or "numpy" (profile.ProfileDP / MergedProfileDP.rowPosteriors, no GPU needed).
    Tensors go through host memory, as pair_profile_loglike's do."""
    if logP.dtype != torch.float64 or logP.dim() != 2:
        raise ValueError("logP is a float64 [sumRows, nOutTok + 1] (merged: [sumRows, nCols + 1]) tensor")
    rowOff = np.asarray(rowOff, np.int64).reshape(-1)
    if len(rowOff) < 1 or rowOff[0] != 0 or rowOff[-1] != logP.shape[0] or (np.diff(rowOff) < 0).any():
        raise ValueError("rowOff has one entry per profile and one more, from 0 up to the rows of logP")
    if colTok is not None:
        colTok = np.asarray(colTok, np.int64).reshape(-1)
        if logP.shape[1] != len(colTok) + 1:
            raise ValueError("merged profiles: logP has one column per entry of colTok and the blank in front")
    return _ProfileLoglike.apply(logP, machine_or_dm, rowOff, colTok, backend)
