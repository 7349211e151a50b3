"""The predicted schedule of LinearMpcZmp on a 16384-bucket key, in two launches: from 131072 QPs (csrc/zmp.hip kRankedMinQp)
zmp_predict_rank_kernel counts and ranks every QP's key in the pass that computes it, and csrc/common.hip
order_place_ranked_kernel places them.  Below that size the three launches on 256 buckets stay (the fused pass costs one
atomic per QP, which only a large batch's better pairs pay for), so the sizes here come in two kinds: those of the issue
(8192, 8193 instances: the three launches) and their counterparts from 65536 instances on (the two launches).

A schedule is never an input of the arithmetic, so every test holds the handle under test -- which must report "predicted
pivot counts" -- to a handle that orders nothing (CCC_ZMP_PREDICT=0, CCC_ZMP_HISTORY=0, schedule "none"): planned ZMP, jerk
and status, pivot counts included, bit for bit.  A QP that the order lost or held twice would show there: its outputs
would stay unwritten (they are pre-filled with NaN / -1) or a neighbour's would.

Chunks: a workgroup of zmp_predict_rank_kernel covers 256 consecutive QPs (eight passes of 32); the grid is the number of
chunks, so no workgroup is without a chunk, but the last one can be nearly empty.  A call has an even number of QPs (two
per instance): "one more / one less than a multiple of the chunk" is two more / two less here."""
import os
import sys

import numpy as np
import pytest

from centroidalcontrolcollection_amd import LinearMpcZmp
from centroidalcontrolcollection_amd import fixtures as fx

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import zmp_schedule_key as sk  # noqa: E402

pytestmark = pytest.mark.gpu


def _handles(monkeypatch, dt, duration=2.0):
    """(the reference that orders nothing, the handle under test: no history, predicted from the smallest size on)"""
    monkeypatch.setenv("CCC_ZMP_PREDICT", "0")
    monkeypatch.setenv("CCC_ZMP_HISTORY", "0")
    plain = LinearMpcZmp(1.0, duration, dt)
    monkeypatch.delenv("CCC_ZMP_PREDICT")
    monkeypatch.setenv("CCC_ZMP_PREDICT_MIN", "1")
    pred = LinearMpcZmp(1.0, duration, dt)
    return plain, pred


def _run(m, x0, zlim, stream=None):
    import torch

    dev = torch.device("cuda:0")
    n, N = zlim.shape[0], zlim.shape[-1]
    tx, tz = torch.from_numpy(x0).to(dev), torch.from_numpy(zlim).to(dev)
    z = torch.full((n, 2), float("nan"), dtype=torch.float64, device=dev)
    j = torch.full((n, 2, N), float("nan"), dtype=torch.float64, device=dev)
    st = torch.full((n, 2), -1, dtype=torch.int32, device=dev)
    m.plan_batch_device(tx, tz, 0.005, z, j, st)
    torch.cuda.synchronize()
    return z.cpu().numpy(), j.cpu().numpy(), st.cpu().numpy()


def _same(plain, pred, x0, zlim):
    ref = _run(plain, x0, zlim)
    assert plain.last_schedule() == "none"
    got = _run(pred, x0, zlim)
    assert pred.last_schedule() == "predicted pivot counts" and pred.last_kernel() == "zmp_plan_kernel<32,2>"
    for a, r in zip(got, ref):
        assert np.array_equal(a, r)  # (no NaN / -1 left either: the reference has none)
    assert not np.isnan(ref[0]).any() and (ref[2] >= 0).all()
    return ref


@pytest.mark.parametrize(
    "n",
    [
        8192,  # 16384 QPs: the default threshold of the prediction (three launches)
        8193,  # odd (three launches)
        65535,  # 131070 QPs: the last size of the three launches
        65536,  # 131072 QPs: the first size of the two launches, 512 whole chunks
        65537,  # two QPs more: the last workgroup has one pair of QPs, fifteen of its sixteen wavefronts none
        65663,  # 131326 QPs: two short of 513 chunks
    ],
)
def test_chunk_edges(n, monkeypatch):
    b = fx.make_zmp_batch(n, 32, 0.0625, seed=700 + n % 97)
    plain, pred = _handles(monkeypatch, 0.0625)
    _same(plain, pred, b["x0"], b["zlim"])
    b2 = fx.make_zmp_batch(n, 32, 0.0625, seed=800 + n % 97)  # (a second call finds the bucket counts clear again)
    _same(plain, pred, b2["x0"], b2["zlim"])


@pytest.mark.parametrize("n", [3001, 3100, 65600])
def test_idle_lanes(n, monkeypatch):
    """N = 13: the lanes of rows 13 .. 31 add nothing to a key.  3001 instances are 6002 QPs, below the 6144 from which a
    call is scheduled at all (csrc/zmp.hip kSchedMinQp, older than the prediction and not lowered by CCC_ZMP_PREDICT_MIN):
    that call must still give the reference's answers, unordered; 3100 instances take the three launches, 65600 the two."""
    N = 13
    dt = 2.0 / N
    b = fx.make_zmp_batch(n, N, dt, seed=913)
    plain, pred = _handles(monkeypatch, dt)
    assert pred.horizon_steps_ == N
    if 2 * n >= 6144:
        _same(plain, pred, b["x0"], b["zlim"])
    else:
        ref, got = _run(plain, b["x0"], b["zlim"]), _run(pred, b["x0"], b["zlim"])
        assert pred.last_schedule() == "none"
        for a, r in zip(got, ref):
            assert np.array_equal(a, r)


@pytest.mark.parametrize("kind", ["all feasible", "all violated"])
def test_degenerate_keys(kind, monkeypatch):
    """Every key the same, so one bucket holds the whole batch (and one counter takes every workgroup's atomic): key 0 when
    the unconstrained optimum of every QP is feasible; the largest key a 32-row horizon has when it violates every row
    (the clamp itself is the limit of an endless horizon, which no batch reaches)."""
    n, N = 65536, 32
    x0 = np.zeros((n, 2, 3))
    zlim = np.empty((n, 2, 2, N))
    if kind == "all feasible":
        zlim[:, :, 0, :], zlim[:, :, 1, :] = -10.0, 10.0
    else:
        zlim[:, :, 0, :], zlim[:, :, 1, :] = 0.01, 0.05
    viol = sk.violated_rows(x0, zlim, 0.0625)
    assert viol.all() == (kind == "all violated") and viol.any() == (kind == "all violated")
    assert len(np.unique(sk.ranked_bucket(viol, 0.0625))) == 1
    plain, pred = _handles(monkeypatch, 0.0625)
    ref = _same(plain, pred, x0, zlim)
    if kind == "all feasible":
        assert (ref[2] == 0).all()  # (solved, no pivot)
    # ... and a mixed batch right after: the one bucket's count was cleared with the rest
    b = fx.make_zmp_batch(n, 32, 0.0625, seed=77)  # (shared size: the handles' buffers are there)
    _same(plain, pred, b["x0"], b["zlim"])


def test_capture(monkeypatch):
    """One eager call at the size, then the call captured on a stream (a single chain: prediction, place pass, solve) and
    replayed on fresh inputs: the place pass leaves the bucket counts clear, so every replay starts as the first call did."""
    import torch

    dev = torch.device("cuda:0")
    n = 65537
    batches = [fx.make_zmp_batch(n, 32, 0.0625, seed=40 + k) for k in range(3)]
    plain, pred = _handles(monkeypatch, 0.0625)
    x0, zlim = torch.from_numpy(batches[0]["x0"]).to(dev), torch.from_numpy(batches[0]["zlim"]).to(dev)
    z = torch.zeros((n, 2), dtype=torch.float64, device=dev)
    j = torch.zeros((n, 2, 32), dtype=torch.float64, device=dev)
    st = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pred.plan_batch_device(x0, zlim, 0.005, z, j, st, s)  # eager: the scheduling buffers grow here
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pred.plan_batch_device(x0, zlim, 0.005, z, j, st, torch.cuda.current_stream())
    assert pred.last_schedule() == "predicted pivot counts"
    for b in batches[1:]:
        x0.copy_(torch.from_numpy(b["x0"]))
        zlim.copy_(torch.from_numpy(b["zlim"]))
        z.fill_(float("nan"))
        j.fill_(float("nan"))
        st.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        got = (z.cpu().numpy(), j.cpu().numpy(), st.cpu().numpy())
        ref = _run(plain, b["x0"], b["zlim"])
        assert plain.last_schedule() == "none"
        for a, r in zip(got, ref):
            assert np.array_equal(a, r)


def test_the_keys_resolution(monkeypatch):
    """What the finer key buys, from the kernel's own pivot counts: the lock-step waste of the pairs made by the key in the
    256 buckets it had (rint(16 sum), as tests/test_zmp_gpu.py writes it) against the same sum in 16384 buckets
    (tests/tools/zmp_schedule_key.py).  Measured on an MI355X on this batch: see DESIGN.md section 4."""
    n = 20000
    b = fx.make_zmp_batch(n, 32, 0.0625, seed=60)
    plain, _ = _handles(monkeypatch, 0.0625)
    piv = (_run(plain, b["x0"], b["zlim"])[2] >> 8).reshape(-1).astype(np.int64)
    viol = sk.violated_rows(b["x0"], b["zlim"], 0.0625)
    i = np.arange(32)
    key = np.rint(16.0 * (viol * np.exp(-i * 0.0625 / (2.35 * np.sqrt(1.0 / 9.80665)))).sum(1))
    parent = piv[np.argsort(-key, kind="stable")].reshape(-1, 2).max(1).sum() * 2.0 / piv.sum()
    assert parent == sk.lockstep_waste(piv, key)
    ranked = sk.lockstep_waste(piv, sk.ranked_bucket(viol, 0.0625))
    print("lock-step waste of the pairs: 256 buckets %.4f, 16384 buckets %.4f" % (parent, ranked))
    assert ranked < parent, (ranked, parent)
