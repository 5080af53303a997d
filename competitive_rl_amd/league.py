"""LeagueEnvWrapper: cPongTournament with an opponent PER ENV, chosen and served on the device.

The reference's ``TournamentEnvWrapper`` (competitive_rl/pong/competitive_pong_env.py:9-53) has one ``current_agent`` for all its envs;
a trainer gets a mixed population of opponents because it runs many worker processes, each drawing its own
(``reset_opponent`` -> ``random.choice(agent_names)``, :27-33).  On this backend one batch is the population, so the league keeps an
int32 ``assignment`` per env on the device (index into ``agent_names``) and serves every env's opponent in the step:

* pool: any of RANDOM, RULE_BASED, WEAK, MEDIUM, plus LightActorCritic weight sets of the caller's own (``add_agent``) and full-size
  ActorCritic weight sets -- the network of the reference's STRONG / ALPHA_PONG and of ``Policy(..., use_light_model=False)``
  (utils/network.py:14-56) -- through ``add_full_agent``: a trainer's own snapshots, served per env like every other agent.  Their
  three kernels run on the agent's env list; the activations between them live in one scratch per league (16.5 KB per row, about
  1.1 GB at 65 536 rows; ``scratch_rows`` trades memory for passes);
* every pool entry carries a play style, ``(temperature, epsilon)`` (``set_sampling`` / ``sampling``; default (0, 0) = greedy, today's
  behaviour): a CNN agent at temperature T samples from the softmax of logits / T as the reference's
  ``Policy.compute_action(obs, deterministic=False)`` does at T = 1 (utils/policy_serving.py:48-56), any agent but RANDOM plays a
  uniform action on a share epsilon of its steps.  The draw is made by the lane that writes the action, in the kernels' epilogues
  (include/crl.h "sampled actions", restated by ``league_sample_reference`` below); the same trained snapshot can sit in a pool
  twice, as the stochastic policy its trainer improves and as its greedy version;
* ``set_opponents`` / ``reset_opponent(name)`` assign, ``reset_opponent()`` draws one opponent per env, ``resample_on_done=True``
  re-draws the opponent of every env whose episode ended, inside the step -- all without a host synchronisation, except
  ``set_opponents`` with one id PER ENV: the wrapper checks the range of those ids on the host before it hands them to the kernels
  (``crl_league_set_assignment`` itself does not wait);
* every draw is Philox4x32-10 keyed by (seed, GLOBAL env id) with a per-env counter (include/crl.h "league draws"), so the result does
  not depend on how a batch is cut into shards.  RANDOM here is therefore ANOTHER stream than the reference's ``np.random.randint(3)``
  (``get_random_policy`` is untouched and still numpy's);
* history: ONE ring of the opponent view's last four frames per env, pushed every step whichever agent is assigned and never cleared at
  episode ends (the rule of ``Policy``'s private stack); every CNN agent reads it.  An env that changes hands is judged on the four
  frames it really showed.  With an assignment that never changes this is ``TournamentEnvWrapper`` with that opponent, bit for bit;
* ``ledger=True`` (or a ``LeagueLedger``) books every finished episode to the opponent that played it, on the device, behind the step;
  with ``resample_on_done`` the next opponent is then the LEDGER's weighted draw (``LeagueLedger.set_weights`` / ``pfsp_weights``)
  instead of the uniform one.  Without a ledger the wrapper runs the launches it always ran;
* ``state_dict()`` / ``load_state_dict()`` (and ``pool_state_dict()`` / ``load_pool_state_dict()`` of the pool alone) hold what a
  continuation needs and the device alone knows -- the act-call and opponent draw counters, the CNN slots' weights as served, the rings,
  the assignment, the books -- so that a league rebuilt in a new process goes on with the draws and actions of the original
  (include/crl.h "checkpoint / resume").

The forward pass, the draws and the partition of the envs by agent are HIP behind ``crl_league_*`` / ``crl_pool_add_full``
(csrc/pong_league.hip, csrc/pong_policy.hip, csrc/pong_policy_full.hip); there is no torch model and no CPU path in this module.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import checkpoint as K
from .ledger import LeagueLedger
from .policy_serving import (_FULL_KEYS, _FULL_SHAPES, _KEYS, _SHAPES, BUILTIN_CHECKPOINTS, Policy, check_full_weights, load_full_weights,
                             load_light_weights)
from .rules import check_sampling, league_draw_reference, league_sample_reference, sample_eps_q  # noqa: F401  (re-exported)
from .tournament import get_builtin_agent_names
from .vec_env import CHEAT_CODES  # noqa: F401  (RULE_BASED's action, written by the fill kernel)

_BUILTIN_KINDS = {"RANDOM": N.CRL_LEAGUE_RANDOM, "RULE_BASED": N.CRL_LEAGUE_RULE_BASED}


def _light_weights(name, source):
    """A LightActorCritic weight set from a checkpoint path, a dict of arrays in torch layout or a light ``Policy``."""
    if isinstance(source, Policy):
        if not source.use_light_model:
            raise ValueError(f"{name}: the full-size ActorCritic is not a LightActorCritic weight set, which is what add_agent takes; "
                             "add_full_agent serves such a policy")
        source = source.weights
    if isinstance(source, str):
        return load_light_weights(source)
    if not isinstance(source, dict):
        raise TypeError(f"{name}: pass a checkpoint path, a dict of LightActorCritic arrays or a light Policy, not {type(source).__name__}")
    if "conv3_w" in source:
        raise ValueError(f"{name}: the full-size ActorCritic is not a LightActorCritic weight set, which is what add_agent takes; "
                         "add_full_agent serves such weights")
    w = {k: np.ascontiguousarray(source[k], np.float32) for k in _KEYS}
    for k in _KEYS:
        if w[k].shape != _SHAPES[k]:
            raise ValueError(f"{name}: {k} has shape {w[k].shape}, LightActorCritic on (4, 42, 42) needs {_SHAPES[k]}")
    return w


def _full_weights(name, source):
    """A full-size ActorCritic weight set (the eight arrays of ``policy_serving._FULL_KEYS``, float32, torch layout) from a checkpoint
    path (``.npz`` or a reference checkpoint), a dict of arrays (further keys, such as the critic's, are ignored) or a full-size
    ``Policy``.  Light weight sets are refused with a pointer to ``add_agent``."""
    if isinstance(source, Policy):
        if source.use_light_model:
            raise ValueError(f"{name}: a LightActorCritic policy is not a full-size ActorCritic; add_agent takes it")
        source = source.weights
    if isinstance(source, str):
        return load_full_weights(source)
    if not isinstance(source, dict):
        raise TypeError(f"{name}: pass a checkpoint path, a dict of ActorCritic arrays or a full-size Policy, not {type(source).__name__}")
    missing = [k for k in _FULL_KEYS if k not in source]
    if missing:
        if "conv3_w" in missing and all(k in source for k in _KEYS):
            raise ValueError(f"{name}: a LightActorCritic weight set (no conv3_w) is not a full-size ActorCritic; add_agent takes it")
        raise ValueError(f"{name}: the full-size ActorCritic needs {list(_FULL_KEYS)}; {missing} are missing")
    for k in _FULL_KEYS:
        if tuple(np.shape(source[k])) != _FULL_SHAPES[k]:
            hint = "; add_agent takes LightActorCritic weight sets" if tuple(np.shape(source[k])) == _SHAPES.get(k) else ""
            raise ValueError(f"{name}: {k} has shape {tuple(np.shape(source[k]))}, ActorCritic on (4, 42, 42) needs {_FULL_SHAPES[k]}{hint}")
    return check_full_weights(source, name)


class AgentPool:
    """What ``LeagueEnvWrapper`` and ``LeagueArena`` (arena.py) both are: a ``crl_league`` handle serving ``rows`` virtual envs, and the
    pool of agents behind it -- names, kinds, play styles, the shared frame rings.  A subclass sets ``device`` and calls ``_open_pool``
    from its constructor; ``_check_new_agent`` and ``_pool_grew`` are its hooks around ``add_agent`` / ``add_full_agent``."""

    def _open_pool(self, rows, env_id_base, seed, agent_names):
        self._rows = int(rows)
        self._L = N.load()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_league_create(self.device.index or 0, self._rows, int(env_id_base), int(seed) & (2 ** 64 - 1), C.byref(h)))
        self._h = h
        self.agent_names, self._kinds = [], []
        for name in get_builtin_agent_names() if agent_names is None else list(agent_names):
            if name in _BUILTIN_KINDS:
                self._add(name, _BUILTIN_KINDS[name])
            elif name in BUILTIN_CHECKPOINTS:
                self._add(name, N.CRL_LEAGUE_LIGHT, load_light_weights(BUILTIN_CHECKPOINTS[name]))
            else:
                raise ValueError("Unknown agent name: {}".format(name))
        if not self.agent_names:
            raise ValueError("the pool is empty")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _add(self, name, kind, weights=None, scratch_rows=None):
        """A builtin, a LightActorCritic or a full-size agent: what the pool refuses is looked at before the library is called."""
        if name in self.agent_names:
            raise ValueError(f"{name} is in the pool already")
        if len(self.agent_names) >= N.CRL_LEAGUE_MAX_AGENTS:
            raise ValueError(f"a pool holds at most {N.CRL_LEAGUE_MAX_AGENTS} agents")
        rows = 0 if scratch_rows is None else int(scratch_rows)
        if scratch_rows is not None and rows <= 0:
            raise ValueError(f"scratch_rows must be positive (None: min(envs, 65536)), not {scratch_rows}")
        with torch.cuda.device(self.device):
            if kind == N.CRL_POOL_KIND_FULL:
                N.check(self._L.crl_pool_add_full(self._h, *[weights[k].ctypes.data_as(C.c_void_p) for k in _FULL_KEYS], rows))
            elif kind == N.CRL_LEAGUE_LIGHT:
                N.check(self._L.crl_league_add_light(self._h, *[weights[k].ctypes.data_as(C.c_void_p) for k in _KEYS]))
            else:
                N.check(self._L.crl_league_add_builtin(self._h, kind))
        self.agent_names.append(name)
        self._kinds.append(kind)

    def _check_new_agent(self, what):
        """Hook: raise if the env cannot take a CNN agent (``what``: its network, for the message)."""

    def _pool_grew(self):
        """Hook: the pool holds one agent more."""

    def _add_cnn(self, name, kind, what, weights_of, source, temperature, epsilon, scratch_rows=None):
        self._check_new_agent(what)
        check_sampling(temperature, epsilon)  # (before the agent enters the pool)
        self._add(name, kind, weights_of(name, source), scratch_rows)
        if temperature or epsilon:
            self.set_sampling(name, temperature, epsilon)
        self._pool_grew()

    def add_agent(self, name, weights_or_checkpoint, temperature=0.0, epsilon=0.0):
        """Beyond the reference: a LightActorCritic agent of one's own -- a checkpoint path (``.npz`` or a reference checkpoint), a
        dict of the six arrays in torch layout, or a light ``Policy`` (a trainer's snapshot).  Future draws include it (in the arena its
        cells enter the draw table with weight 1); the assignment / the pairs in force stay.  Full-size networks are refused here:
        ``add_full_agent`` takes them.  ``temperature`` / ``epsilon``: its play style (``set_sampling``); the default is greedy."""
        self._add_cnn(name, N.CRL_LEAGUE_LIGHT, "LightActorCritic", _light_weights, weights_or_checkpoint, temperature, epsilon)

    def add_full_agent(self, name, weights_or_checkpoint, temperature=0.0, epsilon=0.0, scratch_rows=None):
        """A full-size ActorCritic agent of one's own (utils/network.py:14-56; ``Policy(..., use_light_model=False)``) -- a checkpoint
        path (``.npz`` or a reference checkpoint), a dict of the eight arrays in torch layout, or a full-size ``Policy``.  Future draws
        include it; the assignment / the pairs in force stay.  Its envs see exactly what a dense ``Policy`` of these weights computes on
        the same frames.  ``temperature`` / ``epsilon``: its play style (``set_sampling``).  ``scratch_rows``: rows of the pool's one
        activation scratch (16.5 KB each), shared by all full-size agents and fixed by the first of them; None = min(rows, 65 536) with
        rows the envs of a league and the 2 * num_envs seats of an arena, about 1.1 GB at 65 536.  Fewer rows cost more passes over the
        agent's list in every step."""
        self._add_cnn(name, N.CRL_POOL_KIND_FULL, "ActorCritic", _full_weights, weights_or_checkpoint, temperature, epsilon, scratch_rows)

    def update_agent(self, agent, weights_or_checkpoint):
        """Replaces the weights of CNN agent ``agent`` (a name or an index) in place -- a learner's newer snapshot into the slot of an older
        one, so a full pool can follow a learner (``crl_pool_load_light`` / ``crl_pool_load_full``).  Takes what ``add_agent`` /
        ``add_full_agent`` take, of the slot's own network; a built-in agent and the other network are refused, the pool is then what
        it was.  Ordered on the current stream, no synchronisation: steps enqueued before play the old weights.  Assignment, lists,
        play styles and the shared history are untouched."""
        a = self._agent_index(agent)
        name, kind = self.agent_names[a], self._kinds[a]
        if kind == N.CRL_LEAGUE_LIGHT:
            w, load, keys = _light_weights(name, weights_or_checkpoint), self._L.crl_pool_load_light, _KEYS
        elif kind == N.CRL_POOL_KIND_FULL:
            w, load, keys = _full_weights(name, weights_or_checkpoint), self._L.crl_pool_load_full, _FULL_KEYS
        else:
            raise ValueError(f"{name} is a built-in agent without weights")
        with torch.cuda.device(self.device):
            N.check(load(self._h, a, *[w[k].ctypes.data_as(C.c_void_p) for k in keys], self._stream()))

    def _agent_index(self, agent):
        if isinstance(agent, str):
            if agent not in self.agent_names:
                raise ValueError(f"{agent} is not in the pool {self.agent_names}")
            return self.agent_names.index(agent)
        if not 0 <= int(agent) < len(self.agent_names):
            raise ValueError(f"agent {agent} is not in the pool of {len(self.agent_names)}")
        return int(agent)

    def set_sampling(self, agent, temperature=1.0, epsilon=0.0):
        """The play style of ``agent`` (a name or an index; in the arena: in either seat) from the next step on: ``temperature`` 0 plays
        the argmax, T > 0 samples from softmax(logits / T); ``epsilon``: the share of steps with a uniform action instead (RULE_BASED:
        instead of the cheat code).  Neither has an effect on RANDOM, the temperature none on RULE_BASED.  Host values that travel with
        the next launches: no synchronisation."""
        t, e = check_sampling(temperature, epsilon)
        N.check(self._L.crl_sampling_set_agent(self._h, self._agent_index(agent), t, e))

    def sampling(self):
        """Host dict ``name -> (temperature, epsilon)`` of the whole pool (no GPU work)."""
        out = {}
        for a, name in enumerate(self.agent_names):
            t, e = C.c_float(), C.c_float()
            N.check(self._L.crl_sampling_get_agent(self._h, a, C.byref(t), C.byref(e)))
            out[name] = (t.value, e.value)
        return out

    def get_agent_names(self):
        return self.agent_names

    # ---- the shared history
    def reset_history(self):
        """Zeroes the frame rings (``Policy.reset``)."""
        N.check(self._L.crl_league_reset(self._h, self._stream()))

    def get_stack(self):
        out = torch.empty((self._rows, 4, 42, 42), dtype=torch.uint8, device=self.device)
        N.check(self._L.crl_league_get_stack(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def set_stack(self, stack):
        s = torch.as_tensor(stack).to(self.device, torch.uint8).contiguous()
        assert tuple(s.shape) == (self._rows, 4, 42, 42)
        N.check(self._L.crl_league_set_stack(self._h, C.c_void_p(s.data_ptr()), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()

    # ---- checkpoint / resume: the pool's part (include/crl.h "checkpoint / resume")
    def pool_counters(self, draw_counters=True):
        """(seed, env_id_base, act calls, draw counters): the key of the pool's draws, the global id of row 0, the act-call counter --
        the ``n`` of RANDOM's and of every sampled or explored action -- as host ints, and the per-row opponent draw counters as an
        int32 device tensor holding the uint32 bits (a copy enqueued on the current stream, no synchronisation; None without
        ``draw_counters``: then there is no GPU work at all)."""
        seed, base, calls = C.c_uint64(), C.c_int64(), C.c_uint32()
        ctr = torch.empty((self._rows,), dtype=torch.int32, device=self.device) if draw_counters else None
        N.check(self._L.crl_pool_get_counters(self._h, C.byref(seed), C.byref(base), C.byref(calls), C.c_void_p(ctr.data_ptr()) if draw_counters else None,
                                              self._stream()))
        return seed.value, base.value, calls.value, ctr

    def slot_weights(self, agent):
        """The weights the device serves for CNN agent ``agent`` (a name or an index) right now, read back behind everything enqueued on
        the current stream (a learner's ``push``, ``update_agent``): float32 arrays in torch layout under the keys ``update_agent``
        takes.  SYNCHRONISES with the current stream.  A built-in agent has none."""
        a = self._agent_index(agent)
        if self._kinds[a] not in (N.CRL_LEAGUE_LIGHT, N.CRL_POOL_KIND_FULL):
            raise ValueError(f"{self.agent_names[a]} is a built-in agent without weights")
        layout, floats = K.layout_of(self._kinds[a] == N.CRL_LEAGUE_LIGHT, critic=False)
        blob = np.empty(floats, np.float32)
        with torch.cuda.device(self.device):
            N.check(self._L.crl_pool_get_blob(self._h, a, blob.ctypes.data_as(C.c_void_p), floats, self._stream()))
        return K.split_blob(blob, layout)

    def pool_state_dict(self, stack=True):
        """The pool's state as host arrays (SYNCHRONISES with the current stream): ``agent_names`` and ``kinds``, ``rows``, the ``seed``,
        ``env_id_base``, the act-call counter ``act_calls``, the per-row opponent draw counters ``draw_ctr``, the play styles
        (``sampling``: [temperature, epsilon] rows in pool order), per LIGHT / FULL slot the ``weights`` as the device holds them
        (``slot_weights``) and, with ``stack``, the shared rings as ``get_stack()`` shows them."""
        seed, base, calls, ctr = self.pool_counters()
        styles = self.sampling()
        sd = {"kind": "AgentPool", "rows": self._rows, "agent_names": list(self.agent_names), "kinds": [int(k) for k in self._kinds], "seed": seed,
              "env_id_base": base, "act_calls": calls, "draw_ctr": ctr.cpu().numpy().view(np.uint32),
              "sampling": np.array([styles[n] for n in self.agent_names], np.float32).reshape(-1, 2),
              "weights": {n: self.slot_weights(a) for a, n in enumerate(self.agent_names) if self._kinds[a] in (N.CRL_LEAGUE_LIGHT, N.CRL_POOL_KIND_FULL)}}
        if stack:
            sd["stack"] = self.get_stack().cpu().numpy()
        return sd

    def check_pool_state_dict(self, sd):
        """What ``load_pool_state_dict`` refuses, raised before anything is written: another list of names or kinds, other ``rows`` or
        another ``env_id_base``, counters out of range, a style ``check_sampling`` refuses, a slot's tensor or the rings in a wrong
        shape.  Returns what the load writes."""
        K.check_header(sd, "AgentPool", "the pool", rows=self._rows, agent_names=list(self.agent_names), kinds=[int(k) for k in self._kinds],
                       env_id_base=self.pool_counters(draw_counters=False)[1])
        seed, calls = K.check_counter(sd.get("seed"), 64, "seed", "the pool"), K.check_counter(sd.get("act_calls"), 32, "act_calls", "the pool")
        ctr = K.check_array(sd, "draw_ctr", (self._rows,), 4, "the pool")
        styles = K.check_array(sd, "sampling", (len(self.agent_names), 2), 4, "the pool").view(np.float32)
        styles = [K.check_style(t, e, f"the pool, {n}") for n, (t, e) in zip(self.agent_names, styles)]
        weights = {}
        for a, n in enumerate(self.agent_names):
            if self._kinds[a] in (N.CRL_LEAGUE_LIGHT, N.CRL_POOL_KIND_FULL):
                layout, floats = K.layout_of(self._kinds[a] == N.CRL_LEAGUE_LIGHT, critic=False)
                w = sd.get("weights", {}).get(n) if isinstance(sd.get("weights"), dict) else None
                K.join_blob(w, layout, floats, f"the pool, slot {n}")
                weights[n] = {k: w[k] for k in layout}
        stack = K.check_array(sd, "stack", (self._rows, 4, 42, 42), 1, "the pool") if sd.get("stack") is not None else None
        return seed, calls, ctr, styles, weights, stack

    def load_pool_state_dict(self, sd, styles=True):
        """Puts a ``pool_state_dict()`` back: seed and counters, play styles (unless ``styles`` is false: the arena's own ``sampling``
        key says them), every CNN slot's weights and (if the dict has them) the rings, so that RANDOM, the sampled and explored actions
        and the opponent draws continue where the original's would.  Everything is looked at before anything is written
        (``check_pool_state_dict``): a refused load raises a ``ValueError`` and leaves the pool as it was.  Ordered on the current
        stream and SYNCHRONISES with it."""
        seed, calls, ctr, loaded_styles, weights, stack = self.check_pool_state_dict(sd)
        self._seed_pool(seed)  # (zeroes both counters; they are written below)
        ctr_dev = torch.from_numpy(ctr.view(np.int32).copy()).to(self.device)
        N.check(self._L.crl_pool_set_counters(self._h, calls, C.c_void_p(ctr_dev.data_ptr()), self._stream()))
        for a, (t, e) in enumerate(loaded_styles if styles else ()):
            self.set_sampling(a, t, e)
        for n, w in weights.items():
            self.update_agent(n, w)
        if stack is not None:
            self.set_stack(stack.view(np.uint8))
        torch.cuda.current_stream(self.device).synchronize()  # the staging tensors above are this call's own

    # ---- lifetime: the handle's part
    def _seed_pool(self, seed):
        N.check(self._L.crl_league_seed(self._h, int(seed or 0) & (2 ** 64 - 1), self._stream()))

    def _close_pool(self):
        """Destroys the handle; False if it was closed before."""
        if not getattr(self, "_h", None):
            return False
        torch.cuda.synchronize(self.device)
        self._L.crl_league_destroy(self._h)
        self._h = None
        return True

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.crl_league_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class LeagueEnvWrapper(AgentPool):
    """Same single-agent protocol as ``TournamentEnvWrapper`` (step / step_device / reset / reset_opponent / get_agent_names / seed /
    close); see the module docstring for what differs.  ``env_id_base``: the global id of env 0 (default: the wrapped env's).
    ``ledger``: None (no books), True (the wrapper builds a ``LeagueLedger`` with its own seed and id base, and closes it) or a
    ``LeagueLedger`` of the caller's (used as given, not closed)."""

    def __init__(self, env, num_envs, agent_names=None, seed=0, resample_on_done=False, env_id_base=None, ledger=None):
        self.env, self.num_envs = env, int(num_envs)
        device = getattr(env, "device", None)
        if device is None:
            raise RuntimeError("LeagueEnvWrapper needs the HIP vector env (there is no CPU fallback)")
        self.device = torch.device(device)
        names = get_builtin_agent_names() if agent_names is None else list(agent_names)
        cnn = [n for n in names if n in BUILTIN_CHECKPOINTS]
        if cnn and getattr(env, "R", 42) != 42:
            raise ValueError(f"{cnn} are trained on 42x42 frames (builtin_policies.py:36); make the env with resized_dim=42 "
                             "or pass agent_names without them")
        self.resample_on_done = bool(resample_on_done)
        self.env_id_base = int(getattr(env, "env_id_base", 0) if env_id_base is None else env_id_base)
        self.observation_space, self.action_space = env.observation_space[0], env.action_space[0]
        self.prev_opponent_obs = None  # what the opponents act on: the right-hand view of the previous step / reset
        self.record_logits = False     # tests: keep the CNN agents' logits of every step (``logits()``)
        self._act = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)
        self._logits = torch.zeros((self.num_envs, 3), dtype=torch.float32, device=self.device)
        self._open_pool(self.num_envs, self.env_id_base, seed, names)
        self.set_opponents("RULE_BASED" if "RULE_BASED" in self.agent_names else 0)  # the reference starts with RULE_BASED
        self.ledger, self._own_ledger = None, ledger is True
        if ledger is not None and ledger is not False:
            if ledger is True:
                ledger = LeagueLedger(self.num_envs, len(self.agent_names), self.device, seed=seed, env_id_base=self.env_id_base)
            if not isinstance(ledger, LeagueLedger):
                raise TypeError(f"ledger: None, True or a LeagueLedger, not {type(ledger).__name__}")
            if ledger.num_envs != self.num_envs or ledger.agents != len(self.agent_names) or (ledger.device.index or 0) != (self.device.index or 0):
                raise ValueError(f"ledger: {ledger.num_envs} envs x {ledger.agents} agents on {ledger.device}, the league has "
                                 f"{self.num_envs} x {len(self.agent_names)} on {self.device}")
            self.ledger = ledger
            self._ids = [torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device) for _ in range(2)]  # played / next

    # ---- pool: the hooks
    def _check_new_agent(self, what):
        if getattr(self.env, "R", 42) != 42:
            raise ValueError(f"{what} opponents act on 42x42 frames: make the env with resized_dim=42")

    def _pool_grew(self):
        if self.ledger is not None:
            self.ledger.set_agents(len(self.agent_names))

    # ---- assignment
    def set_opponents(self, ids):
        """``ids``: an agent name or index for every env, or one index per env ((N,) array / tensor; a device tensor stays there).  A name
        or a single index is one launch on the current stream, no synchronisation; per-env ids are range-checked on the host first,
        which SYNCHRONISES with the current stream: not for the hot loop (``ledger.update(..., out=)`` / ``resample_on_done`` redraw there)."""
        if isinstance(ids, str):
            assert ids in self.agent_names, self.agent_names
            ids = self.agent_names.index(ids)
        if isinstance(ids, (int, np.integer)):
            assert 0 <= int(ids) < len(self.agent_names), ids
            N.check(self._L.crl_league_set_assignment(self._h, None, int(ids), self._stream()))
            return
        t = torch.as_tensor(ids).to(self.device, torch.int32).reshape(-1).contiguous()
        if t.numel() != self.num_envs:
            raise ValueError(f"one opponent per env: expected {self.num_envs} ids, got {t.numel()}")
        if int(t.min()) < 0 or int(t.max()) >= len(self.agent_names):
            raise ValueError(f"opponent ids must index agent_names (0..{len(self.agent_names) - 1})")
        N.check(self._L.crl_league_set_assignment(self._h, C.c_void_p(t.data_ptr()), 0, self._stream()))

    def reset_opponent(self, agent_name=None):
        """A name: that opponent for every env (competitive_pong_env.py:27-33).  None: one fresh draw PER ENV, on the device."""
        if agent_name is None:
            N.check(self._L.crl_league_resample(self._h, None, self._stream()))
        else:
            self.set_opponents(agent_name)

    @property
    def assignment(self):
        """int32 (N,) device tensor: a copy of the assignment in force (enqueued on the current stream, no synchronisation)."""
        out = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
        N.check(self._L.crl_league_get_assignment(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def _lists(self, want_lists):
        a = len(self.agent_names)
        counts = torch.zeros((N.CRL_LEAGUE_MAX_AGENTS,), dtype=torch.int32, device=self.device)
        lists = torch.full((a, self.num_envs), -1, dtype=torch.int32, device=self.device) if want_lists else None
        N.check(self._L.crl_league_get_lists(self._h, C.c_void_p(counts.data_ptr()), C.c_void_p(lists.data_ptr()) if want_lists else None,
                                             self._stream()))
        return counts[:a].cpu().numpy().astype(np.int64), lists

    def counts(self):
        """Envs per agent, in ``agent_names`` order (host array; synchronises)."""
        return self._lists(False)[0]

    def agent_lists(self):
        """Debug: {name: env indices the kernels visit for that CNN agent} (sorted host arrays; synchronises)."""
        counts, lists = self._lists(True)
        lists = lists.cpu().numpy()
        return {n: np.sort(lists[a, :counts[a]]) for a, n in enumerate(self.agent_names)
                if self._kinds[a] in (N.CRL_LEAGUE_LIGHT, N.CRL_POOL_KIND_FULL)}

    def logits(self):
        """float32 (N, 3): with ``record_logits`` set, the logits of the last step for envs on a CNN agent (other rows keep what they held)."""
        return self._logits

    # ---- FrameStackTensor binding and early done flags: the wrapped env's, as this wrapper's own hooks
    def _stack_env(self):
        """The env a FrameStackTensor binds to (frame_stack.py): agent 0's observation of the wrapped env is this wrapper's."""
        return getattr(self.env, "_stack_env", lambda: None)()

    def done_host(self):
        """The last step's done flags on the host, ahead of the observation (HipPongVecEnv.done_host)."""
        return self.env.done_host()

    def rule_labels(self, seat=0, out=None):
        """RULE_BASED's next action per env as int32 labels on the device (HipPongVecEnv.rule_labels); seat 0 is the learner's bat."""
        return self.env.rule_labels(seat=seat, out=out)

    # ---- VecEnv protocol, agent 0's view
    def _frames(self, obs):
        if isinstance(obs, np.ndarray):
            obs = torch.from_numpy(np.ascontiguousarray(obs))
        if obs.device != self.device:
            obs = obs.to(self.device)
        if obs.dtype != torch.uint8:  # float32 observations hold 0..255 integers
            obs = obs.to(torch.uint8)
        if obs.shape[-1] != 42 or obs.shape[-2] != 42:
            raise ValueError("the league's frame history holds 42x42 frames: make the env with resized_dim=42")
        obs = obs.reshape(self.num_envs, 42, 42) if obs.dim() != 4 else obs[:, -1]  # the newest plane
        if obs.stride(2) != 1 or obs.stride(1) != 42 or obs.stride(0) % 4 or obs.data_ptr() % 4:
            obs = obs.contiguous()
        return obs

    def _fill_actions(self, mine_i32):
        """column 0 <- the caller's actions, column 1 <- every env's own opponent's, written in place by the league's kernels"""
        self._act[:, 0] = mine_i32
        f = self._frames(self.prev_opponent_obs)
        N.check(self._L.crl_league_act(self._h, C.c_void_p(f.data_ptr()), f.stride(0) if self.num_envs > 1 else 1764,
                                       C.c_void_p(self._act.data_ptr() + 4), 2,
                                       C.c_void_p(self._logits.data_ptr()) if self.record_logits else None, self._stream()))
        return self._act

    def _after_step(self, done_u8, rew_f32=None):
        if self.ledger is not None:
            # the books want the opponent that PLAYED the step: a device-to-device copy of the assignment, taken before any redraw; the
            # ids go straight to crl_league_set_assignment (set_opponents' range check would read them on the host)
            played, nxt = self._ids
            N.check(self._L.crl_league_get_assignment(self._h, C.c_void_p(played.data_ptr()), self._stream()))
            self.ledger.update(played, rew_f32, done_u8, redraw=self.resample_on_done, out=nxt)
            if self.resample_on_done:
                N.check(self._L.crl_league_set_assignment(self._h, C.c_void_p(nxt.data_ptr()), 0, self._stream()))
        elif self.resample_on_done:
            N.check(self._L.crl_league_resample(self._h, C.c_void_p(done_u8.data_ptr()), self._stream()))

    def step(self, action):
        if self.prev_opponent_obs is None:
            raise RuntimeError("reset() the league before its first step")
        if not isinstance(action, torch.Tensor):
            action = torch.as_tensor(np.asarray(action).reshape(-1), dtype=torch.int32)
        obs, rew, done, info = self.env.step(self._fill_actions(action.to(self.device, torch.int32).reshape(-1)))
        self.prev_opponent_obs = obs[1]
        done = done[:, 0] if done.ndim == 2 else done
        if self.ledger is not None:
            self._after_step(torch.as_tensor(done).to(self.device, torch.uint8).contiguous(), torch.as_tensor(rew).to(self.device, torch.float32))
        elif self.resample_on_done:
            self._after_step(torch.as_tensor(done).to(self.device, torch.uint8).contiguous())
        return obs[0], rew[:, 0].reshape(-1, 1), done.reshape(-1, 1), info

    def step_device(self, actions_i32):
        """Hot-loop entry (no host work, no clones, no sync): ``actions_i32`` is an int32 (N,) device tensor; returns the env's device
        buffers (obs (N, 2, K, R, R) -- view 0 is the caller's --, rewards (N, 2), done (N,)) like HipPongVecEnv.step_device.  With
        ``resample_on_done`` the envs whose flag is set get their next opponent behind the step, on the same stream; with a ledger
        the step's results are booked there as well (and that next opponent is the ledger's weighted draw)."""
        if self.prev_opponent_obs is None:
            raise RuntimeError("reset() the league before its first step")
        buf, rew, done = self.env.step_device(self._fill_actions(actions_i32))
        self.prev_opponent_obs = buf[:, 1]
        self._after_step(done, rew)
        return buf, rew, done

    def reset(self, **kwargs):
        views = self.env.reset(**kwargs)
        self.prev_opponent_obs = views[1]
        return views[0]

    def seed(self, s):
        """Seeds the wrapped env and re-keys the league's draws (sampled and explored actions included) and its ledger's (all draw
        counters start over)."""
        self.env.seed(s)
        self._seed_pool(s)
        if self.ledger is not None:
            self.ledger.seed(s)

    # ---- checkpoint / resume
    def state_dict(self):
        """The league's own state as host arrays (SYNCHRONISES with the current stream): the pool (``pool_state_dict()``: names, kinds,
        seed, the act-call and opponent draw counters, play styles, the CNN slots' weights as the device holds them, the rings), the
        ``assignment``, ``resample_on_done``, ``prev_opponent_obs`` -- a host copy of what the opponents act on next: the env's buffers
        are redrawn only by its next step -- and the ledger's ``state_dict()`` when the league has one.  The wrapped env's state is the
        env's own (``env.state_dict()``)."""
        prev = self.prev_opponent_obs
        if prev is not None:
            prev = prev.cpu().numpy() if isinstance(prev, torch.Tensor) else np.array(prev)
        return {"kind": "LeagueEnvWrapper", "num_envs": self.num_envs, "pool": self.pool_state_dict(), "assignment": self.assignment.cpu().numpy(),
                "resample_on_done": self.resample_on_done, "prev_opponent_obs": prev,
                "ledger": None if self.ledger is None else self.ledger.state_dict()}

    def load_state_dict(self, sd):
        """Puts a ``state_dict()`` back into a league built over the same pool (names and kinds in the same order; seeds and weights
        may differ: they are loaded).  Everything is looked at before anything is written: another pool, another ``num_envs``, ids
        outside the pool, an observation or a ring of another shape, books that do not fit raise a ``ValueError`` and leave the league
        and its ledger as they were.  Ordered on the current stream and SYNCHRONISES with it.  ``prev_opponent_obs`` becomes a device
        tensor of the league's own.  The wrapped env is loaded by the caller (``env.load_state_dict``)."""
        K.check_header(sd, "LeagueEnvWrapper", "the league", num_envs=self.num_envs)
        if not isinstance(sd.get("pool"), dict):
            raise K.refuse("the league: the pool's part is missing")
        self.check_pool_state_dict(sd["pool"])
        ids = K.check_array(sd, "assignment", (self.num_envs,), 4, "the league").view(np.int32)
        if ids.min() < 0 or ids.max() >= len(self.agent_names):
            raise K.refuse(f"the league: the assignment must index agent_names (0..{len(self.agent_names) - 1})")
        prev = sd.get("prev_opponent_obs")
        if prev is not None:
            prev = np.ascontiguousarray(prev)
            if prev.ndim not in (3, 4) or prev.shape[0] != self.num_envs or prev.shape[-2:] != (42, 42):
                raise K.refuse(f"the league: prev_opponent_obs of shape {prev.shape}; the opponents act on ({self.num_envs}, K, 42, 42) frames")
        if (sd.get("ledger") is None) != (self.ledger is None):
            raise K.refuse("the league: %s" % ("the state dict has books, this league has no ledger" if self.ledger is None
                                               else "this league has a ledger, the state dict has no books"))
        if self.ledger is not None:
            self.ledger.check_state_dict(sd["ledger"])
        self.load_pool_state_dict(sd["pool"])
        t = torch.from_numpy(ids.copy()).to(self.device)
        N.check(self._L.crl_league_set_assignment(self._h, C.c_void_p(t.data_ptr()), 0, self._stream()))
        self.resample_on_done = bool(sd["resample_on_done"])
        self.prev_opponent_obs = None if prev is None else torch.from_numpy(prev).to(self.device)
        if self.ledger is not None:
            self.ledger.load_state_dict(sd["ledger"])
        torch.cuda.current_stream(self.device).synchronize()  # the staging tensors above are this call's own

    def close(self):
        if self._close_pool():
            if self._own_ledger and self.ledger is not None:
                self.ledger.close()
            self.env.close()
