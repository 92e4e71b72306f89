"""The pipeline with the run formatter off the walk stream (ta_plan_execute_walk /
_format behind align.DevicePipeline): step k's walk runs on the
walk stream, its formatter on the caller's stream beside walk k + 1.

The hazards are ordering hazards, so the shapes are small: at the default depth
3, four batches in turn over 10 steps (four is coprime with the depth: no slot
holds the same batch twice running), each of 64 uniform random local pairs of
256 x 256 at 1/-1/-1 -- about 250 events a pair, several 64-event formatter
rounds.  Every batch holds one pair of score 0 (no event: the formatter writes
the CIGAR of an empty alignment) and one whose query holds '-' (handed back to the fallback walk, which
writes its CIGAR itself: the formatter must skip it).  Every step's results are
snapshotted on the caller's stream right after step(), with no synchronisation
between steps, and compared with the CPU oracle's for that step's own batch: a
formatter that ran before its walk, or after its slot's next fill, shows
another batch's bytes."""
import numpy as np
import pytest

from bioinfo1_amd import synth
from bioinfo1_amd.align import TA_PLAN_CK, TA_PLAN_NO_CK, Aligner, DevicePipeline, DevicePlan
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.gpu

SC = (1, -1, -1)
MODE = 1  # local
P, N, M = 64, 256, 256
BATCHES, STEPS, DEPTH = 4, 10, 3


def _batch(v):
    u = synth.uniform_batch(P, N, M, seed=0xF0A7 + v)
    pairs = [(u.query(p), u.target(p)) for p in range(P)]
    pairs[5 + v] = (b"A" * N, b"C" * M)  # score 0: a walk of no events
    q = bytearray(pairs[20 + v][0])
    for at in (3, 100 + v, N - 2):
        q[at] = ord("-")  # '-' in the query: the couple is handed back to the int32 fill and the one-pair walk
    pairs[20 + v] = (bytes(q), pairs[20 + v][1])
    return synth.from_pairs(pairs)


@pytest.fixture(scope="module")
def batches():
    return [_batch(v) for v in range(BATCHES)]


@pytest.fixture(scope="module")
def device_inputs(batches):
    import torch

    dev = torch.device("cuda", 0)
    ins = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                 for a in (b.qbytes, b.qoff.view(np.int64), b.tbytes, b.toff.view(np.int64))) for b in batches]
    torch.cuda.synchronize()
    return ins


@pytest.fixture(scope="module")
def wants(batches):
    """The oracle's results for each batch, computed once."""
    orc = Oracle()
    want = [orc.align_batch(b, MODE, *SC, True) for b in batches]
    for v, w in enumerate(want):  # the two special pairs are what they are meant to be
        assert w.scores[5 + v] == 0  # (no event: the formatter writes the CIGAR of an empty alignment)
        assert w.scores[20 + v] > 0 and w.cigar_lens[20 + v] > 0
    return want


def _snapshot(plan):
    dst, off = plan.compact_cigars()
    return plan.score.clone(), plan.target_begin.clone(), plan.cigar_len.clone(), dst, off


def _host(snap):
    sc, tb, cl, dst, off = snap
    return (sc.cpu().numpy(), tb.cpu().numpy().view(np.uint32), cl.cpu().numpy().view(np.uint32),
            dst[:int(off[-1])].cpu().numpy().tobytes())


def _check(snaps, wants, what):
    for k, snap in enumerate(snaps):
        sc, tb, cl, cig = _host(snap)
        want = wants[k % BATCHES]
        np.testing.assert_array_equal(sc, want.scores, err_msg=f"{what} step {k}")
        np.testing.assert_array_equal(tb, want.target_begins, err_msg=f"{what} step {k}")
        np.testing.assert_array_equal(cl, want.cigar_lens, err_msg=f"{what} step {k}")
        assert cig == b"".join(want.cigars()), (what, k)


def _two_chunk_budget(batch, flags):
    """A workspace budget under which the plan splits into exactly 2 chunks."""
    al = Aligner(0)
    try:
        whole = DevicePlan(al, batch, MODE, *SC, True, flags=flags)
        total = whole.workspace_bytes
        whole.close()
        for frac in (0.75, 0.7, 0.65, 0.6, 0.55, 0.5):
            p = DevicePlan(al, batch, MODE, *SC, True, flags=flags, workspace_budget=int(total * frac))
            chunks = p.chunks
            p.close()
            if chunks == 2:
                return int(total * frac)
    finally:
        al.close()
    raise AssertionError("no budget splits the plan into 2 chunks")


def _run(batches, device_inputs, flags, budget=0, format_stream=None):
    """-> (slot 0's plan, chunks, format_split, a snapshot per step); the default depth."""
    pipe = DevicePipeline(0, batches[0], MODE, *SC, True, workspace_budget=budget, flags=flags,
                          inputs=device_inputs[0], format_stream=format_stream)
    try:
        assert len(pipe.plans) == DEPTH
        held, snaps = {}, []
        for k in range(STEPS):
            plan = pipe.step(inputs=device_inputs[k % BATCHES])
            assert held.get(id(plan)) != k % BATCHES  # the slot's last batch was another one
            held[id(plan)] = k % BATCHES
            snaps.append(_snapshot(plan))
        pipe.check()
        return pipe.plans[0], pipe.chunks, pipe.format_split, snaps
    finally:
        pipe.close()


def test_checkpoint_walks(batches, device_inputs, wants):
    plan, chunks, split, snaps = _run(batches, device_inputs, TA_PLAN_CK)
    assert plan.ck and plan.walk == 64 and chunks == 1 and split
    assert plan.dual_pairs == P  # every pair in the packed fill, so the '-' pair is handed back
    _check(snaps, wants, "checkpoint walks")


def test_band_walks(batches, device_inputs, wants):
    plan, chunks, split, snaps = _run(batches, device_inputs, TA_PLAN_NO_CK)
    assert plan.blk and not plan.ck and plan.walk == 64 and chunks == 1 and split
    _check(snaps, wants, "band walks")


def test_two_chunks_take_the_combined_path(batches, device_inputs, wants):
    budget = _two_chunk_budget(batches[0], TA_PLAN_CK)
    plan, chunks, split, snaps = _run(batches, device_inputs, TA_PLAN_CK, budget=budget)
    assert plan.ck and chunks == 2 and not split
    _check(snaps, wants, "two chunks")


def test_format_stream_1_gives_the_same_bytes(batches, device_inputs, wants):
    """format_stream=1 (the formatter on the walk stream) against the default on the same inputs."""
    _, _, split1, kept = _run(batches, device_inputs, TA_PLAN_CK, format_stream=1)
    _, _, split0, default = _run(batches, device_inputs, TA_PLAN_CK)
    assert not split1 and split0
    for k, (a, b) in enumerate(zip(kept, default)):
        got, want = _host(a), _host(b)
        for g, w in zip(got[:3], want[:3]):
            np.testing.assert_array_equal(g, w, err_msg=f"step {k}")
        assert got[3] == want[3], k
    _check(kept, wants, "format_stream 1")


def test_ready_event(batches, device_inputs, wants):
    """Each step's inputs are copied into the slot's own input tensors on a copy stream (after a
    delay on that stream, so a fill that did not wait would read the slot's previous batch) and
    the copy's event is passed as ``ready``; the copy itself follows the slot's previous step on
    the caller's stream, its formatter included.  No host synchronisation until every step is
    enqueued."""
    import torch

    cur = torch.cuda.current_stream()
    copy = torch.cuda.Stream()
    slot_in = [tuple(t.clone() for t in device_inputs[BATCHES - 1]) for _ in range(DEPTH)]
    torch.cuda.synchronize()
    pipe = DevicePipeline(0, batches[0], MODE, *SC, True, flags=TA_PLAN_CK, inputs=slot_in[0])
    try:
        assert pipe.format_split
        after, snaps = [], []
        for k in range(STEPS):
            i = k % DEPTH
            if k >= DEPTH:
                copy.wait_event(after[k - DEPTH])  # the slot's previous results were snapshotted
            with torch.cuda.stream(copy):
                torch.cuda._sleep(2_000_000)
                for dst, src in zip(slot_in[i], device_inputs[k % BATCHES]):
                    dst.copy_(src, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record(copy)
            snaps.append(_snapshot(pipe.step(inputs=slot_in[i], ready=ready)))
            ev = torch.cuda.Event()
            ev.record(cur)
            after.append(ev)
        pipe.check()
    finally:
        pipe.close()
    _check(snaps, wants, "ready")
