"""The Pong serving and learner calls on a HELD side stream (include/crl.h: "all device work is ordered on the caller's HIP stream", and
per section "no call synchronises with the host"; the wrappers' docstrings: "no host synchronisation", "ordered on the current stream",
"the arrays are copied before the call returns", "nothing synchronises").

Every other GPU test enqueues the library's work on the legacy default stream, which serialises with itself: a launch or copy that
forgot its stream argument, a wrapper tensor filled on another stream than its consumer's and a host wait inside a call that promises
none are all invisible there.  A trainer runs on torch side streams, which are non-blocking.  The numerics of these calls are pinned
on the default stream elsewhere (float64 references, oracles, goldens); here the same calls, enqueued on a side stream that a delay
kernel holds back and with no host synchronisation in between, must give the SAME BITS as on the default stream with a synchronisation
after every call -- which hands every existing guarantee over to the way the library is meant to be used.  The instrument, the two
runs and the calls of every chain (and the calls left out, with the reason) are in tests/stream_cases.py; figures and findings in
docs/LAB_NOTES_side_stream.md.

    chain 1  Policy, light and full                      test_policy_chain
    chain 2  LeagueEnvWrapper with a ledger              test_league_chain
    chain 3  LeagueArena                                 test_arena_chain
    chain 4  the learner loop, LightPPO and FullPPO      test_learner_chain
    chain 5  HipPongVecEnv alone, wrapped and raw        test_env_chain
    chain 6  server on stream A, learner on stream B     test_handoff_between_two_streams
    chain 7  one call of chain 4 on the wrong stream     test_the_instrument_sees_a_misordered_call
             a host wait inside a held section           test_the_gate_sees_a_host_wait
"""
import time

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import stream_cases as S  # noqa: E402

_refs = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


@pytest.fixture
def side_stream():
    """A torch side stream that the null stream can overtake while it is held (stream_cases.pick_streams)."""
    _need_gpu()
    return S.pick_streams(1)[0]


@pytest.fixture
def two_side_streams():
    _need_gpu()
    return S.pick_streams(2)


def _reference(case):
    """The reference run of a chain: once per process, left unchanged."""
    if case.name not in _refs:
        _refs[case.name] = S.reference_run(case).out
    return _refs[case.name]


def _episode_ends(out, steps):
    """(steps of pass 0, steps of pass 1) with at least one done flag"""
    return tuple(sum(bool(out["%d:step%d.done" % (k, t)].any()) for t in range(steps)) for k in range(2))


def _check(case, stream, t0, steps=None, **kw):
    ref = _reference(case)
    if steps is not None:  # the books, the redraws and the auto-resets of the chain are exercised, in the held pass too
        ends = _episode_ends(ref, steps)
        S.note("chain %s: steps with an episode end: %d in pass 0, %d in the held pass" % (case.name, ends[0], ends[1]))
        assert ends[1] >= 1 and sum(ends) >= 2, ends
    got = S.held_run(case, {"A": stream, "B": stream}, **kw).out
    bad = S.same(ref, got)
    S.note("test %s: wall time %.2f s" % (case.name, time.perf_counter() - t0))
    assert not bad, "differs from the default-stream run: %s" % bad[:12]


@pytest.mark.parametrize("full", [False, True], ids=["light", "full"])
def test_policy_chain(side_stream, full):
    _check(S.PolicyCase(full), side_stream, time.perf_counter())


def test_league_chain(side_stream):
    _check(S.LeagueCase(), side_stream, time.perf_counter(), steps=S.LEAGUE_STEPS)


def test_arena_chain(side_stream):
    _check(S.ArenaCase(), side_stream, time.perf_counter(), steps=S.ARENA_STEPS)


@pytest.mark.parametrize("full", [False, True], ids=["light", "full"])
def test_learner_chain(side_stream, full):
    _check(S.LearnerCase(full), side_stream, time.perf_counter())


@pytest.mark.parametrize("mode", ["wrapped", "raw"])
def test_env_chain(side_stream, mode):
    _check(S.EnvCase(mode), side_stream, time.perf_counter(), steps=S.ENV_STEPS)


def test_handoff_between_two_streams(two_side_streams):
    """The server on stream A, the learner on stream B: A plays and finishes a rollout, B waits for A and -- held -- updates and pushes,
    A waits for B and -- held -- plays on.  The result is the single-stream reference run of chain 4."""
    t0 = time.perf_counter()
    case = S.LearnerCase(False)
    a, b = two_side_streams
    assert a is not b
    ref = _reference(case)
    got = S.held_run(case, {"A": a, "B": b}, handoff=True).out
    bad = S.same(ref, got)
    S.note("test handoff: wall time %.2f s" % (time.perf_counter() - t0))
    assert not bad, "differs from the default-stream run: %s" % bad[:12]


def test_the_gate_sees_a_host_wait(side_stream):
    """The other half of the instrument: a call that makes the host wait for the held stream (here torch's own ``synchronize``, no
    library call) outlasts the delay, and ``held`` names it."""
    rec = S.Recorder("side", {"A": side_stream})
    rec.k = 1
    with pytest.raises(AssertionError, match=r"First call behind which it was complete: waits#1"):
        with rec.on("A"):
            rec.call("enqueues", torch.zeros, (4,), device="cuda")
            rec.call("waits", side_stream.synchronize)
            rec.call("enqueues", torch.zeros, (4,), device="cuda")
    side_stream.synchronize()


def test_the_instrument_sees_a_misordered_call(side_stream):
    """Chain 4 (light) with ONE call on the wrong stream: in the held pass the ``outcome`` of step 3 is issued under the default stream.
    The copy that fills its rewards tensor was enqueued on the held stream just before and has not run, so the call reads what the tensor
    held -- an earlier step's rewards, and any two steps' rewards differ in every env (stream_cases.LearnerCase.build).  Floats only,
    every buffer allocated: nothing out of range is read.  Returns and advantages must now differ from the reference, while what the
    misplaced call does not feed (the pass before it, the observations, actions, log-probs and values of the rollout) is unchanged: a
    forgotten stream argument inside the library would be seen in the same way."""
    t0 = time.perf_counter()
    case = S.LearnerCase(False)
    ref = _reference(case)
    got = S.held_run(case, {"A": side_stream, "B": side_stream}, misorder=True).out
    bad = set(S.same(ref, got))
    S.note("test misordered: wall time %.2f s, %d of %d kept tensors differ" % (time.perf_counter() - t0, len(bad), len(ref)))
    assert "1:all32.returns" in bad and "1:all32.advantages" in bad and "1:all8.returns" in bad and "1:all8.advantages" in bad, sorted(bad)[:12]
    step3 = (got["1:all32.returns"] != ref["1:all32.returns"]).sum().item()
    assert step3 >= S.N, step3  # (the N samples of step 3 at the least: its reward enters its own return in every env)
    assert not [k for k in bad if k.startswith("0:")], sorted(bad)[:12]
    for f in ("obs", "actions", "old_log_probs", "values"):
        assert "1:all32." + f not in bad and "1:all8." + f not in bad, f
