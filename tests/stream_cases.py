"""The instrument and the call chains of tests/test_hip_side_stream.py.

THE INSTRUMENT.  ``held(stream)`` enqueues one single-thread delay kernel (``torch.cuda._sleep``) on ``stream`` and records an event, the
gate, right behind it.  While the gate is incomplete everything enqueued on ``stream`` afterwards sits behind a blocked stream: work
that a call sent to ANY OTHER stream runs ahead of its inputs, and a call that makes the host wait for the stream outlasts the delay.  On
exit, before anything synchronises, ``held`` asserts that the gate is still incomplete -- a condition, not a measurement; the length of
the delay (4 x the chain's own host time in its warm-up pass, at least ``MIN_DELAY_MS``, at most ``MAX_DELAY_MS``) only has to cover
the host's enqueueing.  ``pick_streams`` takes side streams that the null stream can overtake: with four hardware queues a torch
stream may share one with the null stream, and a delay there would block both.

TWO RUNS PER CHAIN, the same objects from the same seeds and the same calls: ``reference_run`` on the default stream with a device
synchronisation after every library call, ``held_run`` on a side stream.  Every chain is run TWICE on its objects: pass 0 is the
warm-up (on the side stream, unheld: module loading, the pinned stage of a weight reload, the growth of a scratch buffer and lazy
attributes may synchronise there; it also gives the host times), pass 1 runs inside ``held``.  What a run keeps -- clones made on the
stream of the call -- is compared bit for bit by ``same``.

THE CHAINS hold only calls whose docstring or header entry promises that they do not synchronise (listed per chain below).  Left out
because they are documented as synchronising: ``RolloutStorage.stats``, ``LightPPO / FullPPO.stats``, ``.weights``, ``.set_weights``,
``Policy.set_stack``, ``compute_action``, ``__call__``, ``AgentPool.set_stack``, ``state_dict`` / ``load_state_dict`` everywhere,
``counters()``, ``weights()``, ``payoff()``, ``play()``, ``counts()``, ``agent_lists()``, ``done_host()``, ``terminal_observation`` with
host indices, ``get_state`` / ``set_state``, ``check()``, ``step_async`` / ``step_wait`` / ``step``, ``RolloutStorage(debug=True)``,
``set_opponents`` with one id per env and ``set_pairs`` (the range of the ids is checked on the host); they run
before pass 0 or after the final synchronisation.  ``reset()`` of the env, the league and the arena, ``seed()`` and the constructors make
no promise and stay in front of the chains as well.  A second reload through one pinned stage waits on the host for the first one's copy
by design (csrc/pong_league.h), so a pass holds one reload per stage and the stream is synchronised between the passes.
"""
import contextlib
import time
import types

import numpy as np
import pytest
import torch

from competitive_rl_amd.arena import LeagueArena
from competitive_rl_amd.league import LeagueEnvWrapper
from competitive_rl_amd.ppo import FullPPO, LightPPO
from competitive_rl_amd.rollout import RolloutBatch, RolloutStorage
from tests import ppo_cases as PL
from tests import ppo_full_cases as PF
from tests.policy_f64_child import full_policy, light_policy
from tests.policy_full_weights import make_weights
from tests.test_hip_league import _env, _learner_actions, _near_the_end
from tests.test_rollout_storage_rules import reset_pattern

N, T = 67, 6
MIN_DELAY_MS, MAX_DELAY_MS, PROBE_MS = 100.0, 500.0, 20.0  # (4 x the longest chain measured is 9 ms: the floor is there for a busy host)
CANDIDATES = 8
NOTES = []  # the figures of docs/LAB_NOTES_side_stream.md, printed by the tests


def note(text):
    NOTES.append(text)
    print("side-stream: " + text)


# ---------------------------------------------------------------------------------------------------------------- the delay
_cal = {}


def cycles_per_ms():
    """``torch.cuda._sleep`` cycles per millisecond, measured once per process on the delay kernel itself between two events."""
    if "cpm" not in _cal:
        torch.cuda._sleep(1000)  # (loads the kernel)
        torch.cuda.synchronize()
        cycles, ms = 1_000_000, 0.0
        for _ in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 2.0:
                break
            cycles *= 8
        assert ms >= 2.0, f"torch.cuda._sleep({cycles}) took {ms} ms: the delay cannot be calibrated"
        _cal["cpm"] = cycles / ms
        note("delay calibration: torch.cuda._sleep(%d) took %.3f ms, %.0f cycles per ms" % (cycles, ms, _cal["cpm"]))
    return _cal["cpm"]


def _enqueue_delay(stream, ms):
    """The delay on ``stream`` and the gate behind it."""
    cycles = int(cycles_per_ms() * ms)
    gate = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        gate.record(stream)
    return gate


class Hold:
    def __init__(self, gate, delay_ms):
        self.gate, self.delay_ms = gate, delay_ms
        self.first = None  # (label, host ms of that call) of the first call behind which the gate was complete

    def after(self, label, ms):
        if self.first is None and self.gate.query():
            self.first = (label, ms)


@contextlib.contextmanager
def held(stream, delay_ms=MIN_DELAY_MS, warm_ms=None):
    """Everything the body enqueues on ``stream`` sits behind a delay of ``delay_ms``; on exit the gate must still be incomplete.
    ``warm_ms``: label -> host ms of the warm-up pass, for the message."""
    hold = Hold(_enqueue_delay(stream, delay_ms), delay_ms)
    yield hold
    done = hold.gate.query()  # before anything synchronises
    if done:
        label, ms = hold.first if hold.first is not None else ("(after the last call)", float("nan"))
        warm = (warm_ms or {}).get(label, float("nan"))
        raise AssertionError("the gate of the held stream completed inside the held section: the host waited for the stream (or for the "
                             "device).  First call behind which it was complete: %s, host time %.3f ms in this pass, %.3f ms in the warm-up "
                             "pass; delay %.0f ms" % (label, ms, warm, hold.delay_ms))


# ---------------------------------------------------------------------------------------------------------------- the stream
_picked = {"tried": 0, "ok": [], "rejected": []}


def _overtakes(stream):
    """Does work on the null stream finish while ``stream`` is held?  A ``fill_`` on the null stream and an event behind it."""
    x = torch.zeros((16,), device="cuda")
    torch.cuda.synchronize()
    gate = _enqueue_delay(stream, PROBE_MS)
    x.fill_(1.0)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.default_stream())
    while not ev.query() and not gate.query():
        pass
    filled = ev.query()
    still_held = not gate.query()
    torch.cuda.synchronize()
    return filled and still_held


def pick_streams(count):
    """``count`` side streams out of at most ``CANDIDATES`` fresh ones, each of which the null stream overtakes while it is held."""
    while len(_picked["ok"]) < count and _picked["tried"] < CANDIDATES:
        s = torch.cuda.Stream()
        k = _picked["tried"]
        _picked["tried"] += 1
        if _overtakes(s):
            _picked["ok"].append(s)
            note("stream candidate %d taken (of %d tried so far)" % (k, _picked["tried"]))
        else:
            _picked["rejected"].append(s)  # (kept: a fresh stream must not be this one again)
            note("stream candidate %d rejected: the null stream did not get past its delay" % k)
    if len(_picked["ok"]) < count:
        pytest.fail("none of %d fresh torch streams could be overtaken by the null stream while it was held (GPU_MAX_HW_QUEUES: a side "
                    "stream that shares its hardware queue with the null stream blocks both): the instrument would be blind" % _picked["tried"])
    return _picked["ok"][:count]


# ---------------------------------------------------------------------------------------------------------------- the recorder
class Recorder:
    """Runs the calls of a chain, times them on the host and keeps clones of what is compared.

    mode "ref": the default stream, a device synchronisation after every call.  mode "side": the streams of ``streams`` (name ->
    stream); pass 1 holds them."""

    def __init__(self, mode, streams=None):
        self.mode, self.streams = mode, streams or {}
        self.out, self.ms, self.where = {}, [{}, {}], {}
        self.k, self.count, self.hold, self.delay_ms = 0, 0, None, MIN_DELAY_MS

    def begin_pass(self, k):
        self.k, self.count = k, 0
        if k == 1 and self.mode == "side":
            total = sum(self.ms[0].values())
            self.delay_ms = float(min(MAX_DELAY_MS, max(MIN_DELAY_MS, 10.0 * np.ceil(4.0 * total / 10.0))))

    def call(self, name, fn, *args, **kw):
        label = "%s#%d" % (name, self.count)
        self.count += 1
        t0 = time.perf_counter()
        res = fn(*args, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        self.ms[self.k][label] = ms
        if self.mode == "ref":
            torch.cuda.synchronize()
        elif self.hold is not None:
            self.hold.after(label, ms)
        return res

    def keep(self, name, t):
        """A clone on the current stream (torch's own copy: not a call of the chain)."""
        key = "%d:%s" % (self.k, name)
        assert key not in self.out, key
        self.out[key], self.where[key] = t.clone(), torch.cuda.current_stream()

    def keep_batch(self, name, batch):
        for f, t in zip(RolloutBatch._fields, batch):
            self.keep(name + "." + f, t)

    # ---- streams: no-ops in the reference run
    @contextlib.contextmanager
    def on(self, stream, hold=True):
        """The body's calls go to stream ``stream``; in pass 1 it is held (unless ``hold`` is False)."""
        if self.mode == "ref":
            yield
            return
        s = self.streams[stream]
        with torch.cuda.stream(s):
            if self.k == 1 and hold:
                assert self.hold is None
                with held(s, self.delay_ms, self.ms[0]) as h:
                    self.hold = h
                    try:
                        yield
                    finally:
                        self.hold = None
            else:
                yield

    def wait(self, stream, other):
        if self.mode == "side" and self.streams[stream] is not self.streams[other]:
            self.streams[stream].wait_stream(self.streams[other])

    @contextlib.contextmanager
    def misordered(self):
        """The body's calls go to the DEFAULT stream, whatever stream is current (the misordered-call test)."""
        if self.mode == "ref":
            yield
            return
        with torch.cuda.stream(torch.cuda.default_stream()):
            yield

    def reserve(self):
        """Pass 1 keeps as many clones as pass 0 did, and pass 0's are still alive: blocks of their sizes are put into the caching
        allocator's pool of the stream each clone was made on, so that no clone of the held pass has to ask the driver for memory."""
        blocks = []
        for key, t in self.out.items():
            with torch.cuda.stream(self.where[key]):
                blocks.append(torch.empty_like(t))
        del blocks

    def host_ms(self, k):
        return sum(self.ms[k].values())


def same(a, b):
    """Two runs kept the same names, shapes, dtypes and BITS (floats through their int32 views).  Returns the names that differ."""
    assert sorted(a) == sorted(b), (sorted(set(a) ^ set(b)))
    bad = []
    for key in sorted(a):
        x, y = a[key], b[key]
        if isinstance(x, torch.Tensor):
            ok = x.shape == y.shape and x.dtype == y.dtype
            if ok and x.is_floating_point():
                x, y = x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.contiguous().view(
                    torch.int32 if y.dtype == torch.float32 else torch.int64)
            ok = ok and bool(torch.equal(x, y))
        else:
            x, y = np.asarray(x), np.asarray(y)
            ok = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        if not ok:
            bad.append(key)
    return bad


def _run(case, rec, **kw):
    o = case.build()
    torch.cuda.synchronize()  # every input is on the device
    try:
        for k in range(2):
            rec.begin_pass(k)
            case.chain(rec, o, k, **kw)
            if rec.mode == "side":
                for s in rec.streams.values():  # (the passes are separate: pass 0's reload has left its stage)
                    s.synchronize()
                if k == 0:
                    rec.reserve()
        torch.cuda.synchronize()
        rec.k = 2
        case.finish(rec, o)
    finally:
        torch.cuda.synchronize()
        case.close(o)
    return rec


def reference_run(case):
    return _run(case, Recorder("ref"))


def held_run(case, streams, **kw):
    rec = _run(case, Recorder("side", streams), **kw)
    note("chain %s%s: host time of the warm-up pass %.2f ms, of the held pass %.2f ms, delay %.0f ms" % (
        case.name, "".join(" %s=%s" % kv for kv in sorted(kw.items())), rec.host_ms(0), rec.host_ms(1), rec.delay_ms))
    return rec


# ---------------------------------------------------------------------------------------------------------------- pre-roll
_t0 = {}


def preroll_steps(case, steps):
    """Episodes must end INSIDE a chain of ``steps`` steps per pass: a throwaway twin of the case's objects is stepped ``HORIZON`` times
    on the default stream and the start t0 is taken whose window [t0, t0 + 2 * steps) holds the most steps with an episode end, at
    least one of them in the held half.  ``build`` then steps its objects t0 times before the chain (same seeds, same actions)."""
    if case.name not in _t0:
        horizon = 400
        o = case.build(preroll=0)
        done = torch.stack([case.advance(o, t).clone() for t in range(horizon)]).cpu().numpy().astype(bool).any(1)
        case.close(o)
        best = None
        for t0 in range(0, horizon - 2 * steps):
            first, second = int(done[t0:t0 + steps].sum()), int(done[t0 + steps:t0 + 2 * steps].sum())
            if second >= 1 and (best is None or first + second > best[0]):
                best = (first + second, t0)
        assert best is not None, "no episode ended within %d scouted steps" % horizon
        _t0[case.name] = best[1]
        note("chain %s: pre-roll of %d steps, %d of the %d chain steps end an episode in the scouted run" % (case.name, best[1], best[0], 2 * steps))
    return _t0[case.name]


def _overwrite(dst, src=None):
    """Host arrays overwritten IN PLACE right after the call that took them (with ``src``'s values, or with zeros)."""
    for key in dst:
        dst[key][...] = 0 if src is None else src[key]


# ================================================================================================================ chain 1: Policy
class PolicyCase:
    """Policy, light and full.  Calls of a pass: reset, act_device x 2 (a strided column of an (N, 2) tensor; logits), act_rollout x 2
    (reset flags, logits), load_weights(B) -- B's arrays overwritten on the host right after --, act_rollout x 2, get_stack.
    ``set_sampling`` (host values only) is made in front of the chain."""

    def __init__(self, full):
        self.full, self.name = full, "policy-" + ("full" if full else "light")

    def build(self):
        o = types.SimpleNamespace()
        base, pert = (PF.base_weights(), PF.perturbed) if self.full else (PL.base_weights(), PL.perturbed)
        o.A = base
        o.B = [pert(base, 0.05, seed=7 + k) for k in range(2)]
        o.pol = (full_policy if self.full else light_policy)(base, N)
        o.pol.set_sampling(1.0, 0.1, seed=3)
        rs = np.random.RandomState(17)
        o.frames = torch.from_numpy(rs.randint(0, 256, (2, 6, N, 1, 42, 42)).astype(np.uint8)).cuda()
        flags = reset_pattern("random", 2 * 4, N, 5).reshape(2, 4, N)
        o.flags = torch.from_numpy(flags).cuda()
        o.flags_u8 = o.flags.to(torch.uint8) * 5  # (any non-zero byte)
        o.acts2 = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        return o

    def _rollout(self, rec, o, k, i, j):
        pol = o.pol
        reset = o.flags[k, j] if j % 2 else o.flags_u8[k, j]
        values, actions, logp = rec.call("act_rollout", pol.act_rollout, o.frames[k, i], reset=reset, out=o.acts2[:, 0], want_logits=True)
        for name, t in (("values", values), ("actions", actions), ("logp", logp), ("logits", pol.logits())):
            rec.keep("rollout%d.%s" % (j, name), t)

    def chain(self, rec, o, k):
        pol = o.pol
        with rec.on("A"):
            rec.call("reset", pol.reset)
            for i in range(2):
                a = rec.call("act_device", pol.act_device, o.frames[k, i], out=o.acts2[:, 1], want_logits=True)
                rec.keep("act%d.actions" % i, a)
                rec.keep("act%d.logits" % i, pol.logits())
            for j in range(2):
                self._rollout(rec, o, k, 2 + j, j)
            rec.call("load_weights", pol.load_weights, o.B[k])
            _overwrite(o.B[k], o.A)  # "the arrays are copied before the call returns": the calls below must still serve B
            for j in range(2, 4):
                self._rollout(rec, o, k, 2 + j, j)
            rec.keep("stack", rec.call("get_stack", pol.get_stack))

    def finish(self, rec, o):
        pass

    def close(self, o):
        o.pol.close()


# ================================================================================================================ chain 2: league
TABLE = [np.array(t, np.uint32) for t in ([3, 1, 2, 5], [1, 4, 1, 2])]
LEAGUE_STEPS = 12


class LeagueCase:
    """LeagueEnvWrapper with a ledger over RULE_BASED, WEAK, MEDIUM and a full-size agent (scratch of 16 rows: five passes over 67
    envs), MEDIUM sampled, resample_on_done, record_logits.  Calls of a pass: ``reset_opponent()`` (a draw per env), then step_device
    x 12 (crl_league_act, the env's step, the ledger's update, set_assignment) with ``assignment`` after each; after step 1
    ``set_sampling`` of WEAK (host values that travel with the launches), after step 3 ``ledger.set_weights`` (the host table
    overwritten right after), after step 5 ``update_agent`` of the FULL slot from host arrays (4 MB through the pinned stage; the arrays
    overwritten right after), after step 7 ``LightPPO.push`` into MEDIUM, after step 8 ``FullPPO.push`` into FULL, after step 9
    ``ledger.pfsp_weights`` (pass 0: the ledger's own counters, pass 1: ``counters=`` a device tensor); then ``set_opponents(name)``,
    ``assignment``, ``counters_device``, ``weights_device``, the ledger's ``env_state`` and the pool's ``get_stack``.
    Left out: ``set_opponents`` with one id per env -- it checks the range of the ids on the host (documented so in league.py)."""
    name = "league"

    def build(self, preroll=None):
        o = types.SimpleNamespace()
        lg = LeagueEnvWrapper(_env(N, 21), N, ["RULE_BASED", "WEAK", "MEDIUM"], seed=5, resample_on_done=True, ledger=True)
        o.lg = lg
        lg.add_full_agent("FULL", make_weights(2024), scratch_rows=16)
        lg.set_sampling("MEDIUM", 1.0, 0.1)
        lg.record_logits = True
        lg.ledger.set_weights([2, 3, 1, 3])
        lg.reset()
        _near_the_end(lg.env)
        lg.reset_opponent()
        o.acts = _learner_actions(400 + 2 * LEAGUE_STEPS, N, 31)
        o.lr = LightPPO(PL.perturbed(PL.base_weights(), 0.05, seed=11), **PL.HYPER)
        o.lrf = FullPPO(make_weights(7), scratch_rows=64, **PL.HYPER)
        o.tables = [t.copy() for t in TABLE]
        o.W = [{key: x for key, x in make_weights(20 + k).items() if not key.startswith("critic")} for k in range(2)]
        o.t0 = preroll_steps(self, LEAGUE_STEPS) if preroll is None else preroll
        for t in range(o.t0):
            self.advance(o, t)
        return o

    def advance(self, o, t):
        return o.lg.step_device(o.acts[t])[2]

    def chain(self, rec, o, k):
        lg = o.lg
        with rec.on("A"):
            rec.call("reset_opponent", lg.reset_opponent)
            for t in range(LEAGUE_STEPS):
                buf, rew, done = rec.call("step_device", lg.step_device, o.acts[o.t0 + k * LEAGUE_STEPS + t])
                for name, x in (("obs", buf), ("rew", rew), ("done", done), ("logits", lg.logits())):
                    rec.keep("step%d.%s" % (t, name), x)
                rec.keep("step%d.assignment" % t, rec.call("assignment", lambda: lg.assignment))
                if t == 1:
                    rec.call("set_sampling", lg.set_sampling, "WEAK", 1.0 - 0.5 * k, 0.05 + 0.05 * k)
                elif t == 3:
                    rec.call("ledger.set_weights", lg.ledger.set_weights, o.tables[k])
                    o.tables[k][...] = 7
                elif t == 5:
                    rec.call("update_agent", lg.update_agent, "FULL", o.W[k])
                    _overwrite(o.W[k])
                elif t == 7:
                    rec.call("push", o.lr.push, lg, "MEDIUM")
                elif t == 8:
                    rec.call("push(full)", o.lrf.push, lg, "FULL")
                elif t == 9 and k == 0:
                    rec.call("ledger.pfsp_weights", lg.ledger.pfsp_weights, "hard", 2, 1)
                elif t == 9:
                    c = rec.call("counters_device", lg.ledger.counters_device)
                    rec.call("ledger.pfsp_weights(counters)", lg.ledger.pfsp_weights, "variance", 2, 1, counters=c)
            rec.call("set_opponents", lg.set_opponents, "WEAK")
            rec.keep("assignment", rec.call("assignment", lambda: lg.assignment))
            rec.keep("counters", rec.call("counters_device", lg.ledger.counters_device))
            rec.keep("weights", rec.call("weights_device", lg.ledger.weights_device))
            for name, x in zip(("ret", "len", "draw_ctr"), rec.call("env_state", lg.ledger.env_state)):
                rec.keep("ledger." + name, x)
            rec.keep("history", rec.call("get_stack", lg.get_stack))

    def finish(self, rec, o):
        rec.out["env_state"] = o.lg.env.get_state()

    def close(self, o):
        o.lr.close(), o.lrf.close()
        o.lg.close()


# ================================================================================================================ chain 3: arena
ARENA_STEPS = 12


class ArenaCase:
    """LeagueArena over RULE_BASED, WEAK, MEDIUM (sampled), redraw_on_done.  Calls of a pass: step_device x 12 (crl_league_act for both
    seats, the env's step, the books' update, set_assignment) with ``pairs`` after each; after step 4 ``draw_pairs`` (``ArenaBooks.draw``),
    after step 2 ``update_agent`` of WEAK from host arrays (overwritten right after), after step 6 ``set_weights`` (host table,
    overwritten right after), after step 8 ``balance_weights`` (pass 0: the books' own counters, pass 1: ``counters=`` a device tensor),
    after step 10 ``set_sampling`` of WEAK; then ``counters_device``, the books' ``weights_device`` and ``env_state`` and both seats'
    ``get_stack``.  Left out: ``set_pairs`` -- it checks the range of the ids on the host."""
    name = "arena"

    def build(self, preroll=None):
        o = types.SimpleNamespace()
        ar = LeagueArena(_env(N, 23), N, ["RULE_BASED", "WEAK", "MEDIUM"], seed=9)
        o.ar = ar
        ar.set_sampling("MEDIUM", 1.0, 0.1)
        assert ar.redraw_on_done
        ar.reset()
        _near_the_end(ar.env)
        ar.draw_pairs()
        ar.record_logits = True
        o.tables = [np.array(t, np.uint32) for t in ([[0, 3, 1], [2, 0, 5], [1, 1, 0]], [[0, 1, 4], [1, 0, 1], [6, 2, 0]])]
        o.W = [PL.perturbed(PL.base_weights(), 0.05, seed=20 + k) for k in range(2)]
        o.t0 = preroll_steps(self, ARENA_STEPS) if preroll is None else preroll
        for t in range(o.t0):
            self.advance(o, t)
        return o

    def advance(self, o, t):
        return o.ar.step_device()[2]

    def chain(self, rec, o, k):
        ar = o.ar
        with rec.on("A"):
            for t in range(ARENA_STEPS):
                buf, rew, done = rec.call("step_device", ar.step_device)
                for name, x in (("obs", buf), ("rew", rew), ("done", done), ("actions", ar.last_actions), ("logits", ar.logits())):
                    rec.keep("step%d.%s" % (t, name), x)
                rec.keep("step%d.pairs" % t, rec.call("pairs", lambda: ar.pairs))
                if t == 2:
                    rec.call("update_agent", ar.update_agent, "WEAK", o.W[k])
                    _overwrite(o.W[k])
                elif t == 4:
                    rec.call("draw_pairs", ar.draw_pairs)
                elif t == 6:
                    rec.call("set_weights", ar.set_weights, o.tables[k])
                    o.tables[k][...] = 9
                elif t == 8 and k == 0:
                    rec.call("balance_weights", ar.balance_weights)
                elif t == 8:
                    c = rec.call("counters_device", ar.counters_device)
                    rec.call("balance_weights(counters)", ar.balance_weights, 2, c)
                elif t == 10:
                    rec.call("set_sampling", ar.set_sampling, "WEAK", 1.0 - 0.5 * k, 0.05 + 0.05 * k)
            rec.keep("counters", rec.call("counters_device", ar.counters_device))
            rec.keep("weights", rec.call("weights_device", ar.books.weights_device))
            for name, x in zip(("ret", "len", "draw_ctr"), rec.call("env_state", ar.books.env_state)):
                rec.keep("books." + name, x)
            rec.keep("history", rec.call("get_stack", ar.get_stack))

    def finish(self, rec, o):
        rec.out["env_state"] = o.ar.env.get_state()

    def close(self, o):
        o.ar.close()


# ================================================================================================================ chain 5: the env alone
ENV_STEPS = 20


class EnvCase:
    """HipPongVecEnv alone, wrapped mode with frame_stack=4 or raw mode (delta draw: the record of each buffer, its stamp, the fused
    step).  Calls of a pass: step_device x 20 -- step 5j + 2 with ``obs_out=`` a caller tensor, step 5j + 3 with ``render=False`` --, after
    step 5j + 4 ``obs_descriptors`` and ``render_descriptors`` of them, after step 5j + 1 ``terminal_observation`` of five envs by DEVICE
    index.  ``reset()`` promises nothing about synchronisation and is made in front of the chain."""

    def __init__(self, mode):
        self.mode, self.name = mode, "env-" + mode

    def build(self, preroll=None):
        import competitive_rl_amd as crl

        o = types.SimpleNamespace()
        kw = dict(resized_dim=42, frame_stack=4) if self.mode == "wrapped" else {}
        env = crl.HipPongVecEnv(N, seed=3, mode=self.mode, **kw)
        o.env = env
        env.reset()
        _near_the_end(env)
        g = torch.Generator(device="cuda").manual_seed(41)
        o.acts = torch.randint(0, 3, (400 + 2 * ENV_STEPS, N, 2), generator=g, device="cuda", dtype=torch.int32)
        o.mine = torch.zeros(env._obs_shape, dtype=env._buf_dtype, device="cuda")
        o.idx = torch.tensor([0, 13, 31, 64, 66], dtype=torch.int64, device="cuda")
        o.t0 = preroll_steps(self, ENV_STEPS) if preroll is None else preroll
        for t in range(o.t0):
            self.advance(o, t)
        return o

    def advance(self, o, t):
        return o.env.step_device(o.acts[t])[2]

    def chain(self, rec, o, k):
        env = o.env
        with rec.on("A"):
            for t in range(ENV_STEPS):
                a = o.acts[o.t0 + k * ENV_STEPS + t]
                if t % 5 == 2:
                    buf, rew, done = rec.call("step_device(obs_out)", env.step_device, a, obs_out=o.mine)
                elif t % 5 == 3:
                    buf, rew, done = rec.call("step_device(render=False)", env.step_device, a, render=False)
                else:
                    buf, rew, done = rec.call("step_device", env.step_device, a)
                if t % 5 != 3:
                    rec.keep("step%d.obs" % t, buf)
                rec.keep("step%d.rew" % t, rew)
                rec.keep("step%d.done" % t, done)
                if t % 5 == 4:
                    d = rec.call("obs_descriptors", env.obs_descriptors)
                    rec.keep("step%d.descriptors" % t, d)
                    rec.keep("step%d.rendered" % t, rec.call("render_descriptors", env.render_descriptors, d))
                elif t % 5 == 1:
                    for e, views in enumerate(rec.call("terminal_observation", env.terminal_observation, o.idx)):
                        for v, x in enumerate(views):
                            rec.keep("step%d.terminal%d.%d" % (t, e, v), x)

    def finish(self, rec, o):
        rec.out["env_state"] = o.env.get_state()

    def close(self, o):
        o.env.close()


# ================================================================================================================ chain 4: the learner loop
EPOCHS, BATCHES = 2, 3


class LearnerCase:
    """The learner loop, LightPPO or FullPPO(scratch_rows=64: a minibatch of 134 samples runs in three chunks).  Calls of a pass:
    begin(policy) [Policy.get_stack, crl_rollout_begin]; T x (act_rollout, record, outcome -- the rewards through column 0 of an (N, 2)
    tensor); finish(last_values) with normalisation; gather of all samples as float32 and as uint8 and of two fields into a caller's batch;
    minibatches(4, generator);
    update(storage, 2, 3, generator) [randperm, grad, step]; grad of a fixed batch (its views kept) and step; push(policy); act_rollout;
    begin() (carry) and a second rollout, finish and gather.

    ``handoff``: the server's calls go to stream "A", the learner's (update .. push) to stream "B" behind ``B.wait_stream(A)``, the
    server plays on behind ``A.wait_stream(B)``; in pass 1 B and then A are held.  ``misorder``: in pass 1 the outcome of step 3 of
    the first rollout is issued under the DEFAULT stream while the copy that fills its rewards tensor waits on the held stream."""

    def __init__(self, full):
        self.full, self.name = full, "learner-" + ("full" if full else "light")

    def build(self):
        o = types.SimpleNamespace()
        w = PF.base_weights() if self.full else PL.base_weights()
        seed = 41 + self.full
        rs = np.random.RandomState(seed)
        o.pol = (full_policy if self.full else light_policy)(w, N)
        o.pol.set_sampling(1.0, 0.0, seed=seed)
        o.st = RolloutStorage(T, N, normalize_advantage=True)
        o.lr = FullPPO(w, scratch_rows=64, **PL.HYPER) if self.full else LightPPO(w, **PL.HYPER)
        o.gen = torch.Generator(device="cuda")
        steps = 2 * T + 1  # per pass: two rollouts and the call behind the push
        o.frames = torch.from_numpy(rs.randint(0, 256, (2, steps, N, 1, 42, 42)).astype(np.uint8)).cuda()
        flags = reset_pattern("random", 2 * steps, N, seed).reshape(2, steps, N)
        o.flags = torch.from_numpy(flags).cuda()
        o.flags_u8 = o.flags.to(torch.uint8) * 5
        rewards = rs.standard_normal((2, 2 * T, N, 2)).astype(np.float32)
        col = rewards[..., 0].reshape(-1, N)
        assert all(len(np.unique(col[:, e])) == len(col) for e in range(N))  # any two steps' rewards differ in EVERY env
        o.rewards = torch.from_numpy(rewards).cuda()
        o.dones = torch.from_numpy(rs.random_sample((2, 2 * T, N)) < 0.2).cuda()
        o.last = torch.from_numpy(rs.standard_normal((2, 2, N)).astype(np.float32)).cuda()
        o.all = torch.from_numpy(rs.permutation(T * N).astype(np.int64)).cuda()
        o.some = o.all[:150].clone()
        o.acts2 = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
        o.rew2 = torch.zeros((N, 2), dtype=torch.float32, device="cuda")
        return o

    def _rollout(self, rec, o, k, r, misorder):
        """rollout r (0 / 1) of pass k: T x (act_rollout, record, outcome)"""
        pol, st = o.pol, o.st
        for t in range(T):
            i, j = r * (T + 1) + t, r * T + t
            reset = o.flags[k, i] if t % 2 else o.flags_u8[k, i]
            values, actions, logp = rec.call("act_rollout", pol.act_rollout, o.frames[k, i], reset=reset, out=o.acts2[:, 0])
            rec.call("record", st.record, o.frames[k, i], reset, values, actions, logp)
            o.rew2.copy_(o.rewards[k, j])  # (on the current stream)
            if misorder and k == 1 and r == 0 and t == 3:
                with rec.misordered():
                    rec.call("outcome(misordered)", st.outcome, o.rew2[:, 0], o.dones[k, j])
            else:
                rec.call("outcome", st.outcome, o.rew2[:, 0], o.dones[k, j])

    def chain(self, rec, o, k, handoff=False, misorder=False):
        pol, st, lr = o.pol, o.st, o.lr
        o.gen.manual_seed(100 + k)
        with rec.on("A", hold=not handoff):
            rec.call("begin", st.begin, pol)
            self._rollout(rec, o, k, 0, misorder)
            rec.call("finish", st.finish, o.last[k, 0])
            rec.keep_batch("all32", rec.call("gather", st.gather, o.all))
            rec.keep_batch("all8", rec.call("gather(uint8)", st.gather, o.all, obs_dtype=torch.uint8))
            part = rec.call("gather(out)", st.gather, o.some, out=st.empty_batch(o.some.numel(), fields=("returns", "advantages")))
            rec.keep("some.returns", part.returns)
            rec.keep("some.advantages", part.advantages)
            for b, batch in enumerate(rec.call("minibatches", lambda: list(st.minibatches(4, o.gen)))):
                rec.keep_batch("mini%d" % b, batch)
        rec.wait("B", "A")
        with rec.on("B" if handoff else "A"):
            rec.call("update", lr.update, st, EPOCHS, BATCHES, o.gen)
            for key, g in sorted(rec.call("grad", lr.grad, st, o.some).items()):
                rec.keep("grad." + key, g)
            rec.call("step", lr.step)
            rec.call("push", lr.push, pol)
        rec.wait("A", "B")
        with rec.on("A"):
            i = T
            values, actions, logp = rec.call("act_rollout", pol.act_rollout, o.frames[k, i], reset=o.flags[k, i], out=o.acts2[:, 0], want_logits=True)
            for name, x in (("values", values), ("actions", actions), ("logp", logp), ("logits", pol.logits())):
                rec.keep("pushed." + name, x)
            rec.call("begin(carry)", st.begin)
            self._rollout(rec, o, k, 1, False)
            rec.call("finish", st.finish, o.last[k, 1])
            rec.keep_batch("second", rec.call("gather(uint8)", st.gather, o.all, obs_dtype=torch.uint8))

    def finish(self, rec, o):
        for key, x in o.lr.weights().items():
            rec.out["weights." + key] = x
        rec.out["ppo_stats"] = np.array(tuple(o.lr.stats()), np.float64)
        rec.out["rollout_stats"] = np.array(o.st.stats(), np.float64)

    def close(self, o):
        o.lr.close(), o.st.close(), o.pol.close()
