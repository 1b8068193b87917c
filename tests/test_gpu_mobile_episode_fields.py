"""GPU: the episode fields (EpisodeStats: Monitor's accounting) every MobileRobot kernel family leaves behind are the fields that the
same steps leave as launching single steps — exactly.  The other suites pin observations, rewards, dones and the state per kernel;
these six fields they pin only through the per-step entry point and the Monitor files.

MobileRobotGymEnv-v0, discrete actions, 70 envs (one full wavefront and a partial one) x 260 steps (the reset of step 251 falls
inside the call), then a second call of 5 steps in which no episode ends: it must leave last_return / last_length untouched."""
import numpy as np
import pytest

from srlhip import _lib

pytestmark = pytest.mark.gpu

N, T, T2, SEED = 70, 260, 5, 11
FIELDS = {"ep_return": _lib.F_EP_RETURN, "ep_length": _lib.F_EP_LENGTH, "last_return": _lib.F_LAST_RETURN,
          "last_length": _lib.F_LAST_LENGTH, "n_finished": _lib.F_N_FINISHED, "last_reward": _lib.F_LAST_REWARD}


def _handle(rng_mode):
    cfg = _lib.default_config(_lib.ENV_MOBILE)
    cfg.num_envs, cfg.seed0, cfg.rng_mode = N, SEED, rng_mode
    h = _lib.Handle(cfg)
    h.reset()
    return h


def _fields(h):
    return {k: h.get_state(f) for k, f in FIELDS.items()}


def _single_steps(rng_mode, actions):
    """the twin: one launching step per row of `actions` -> the fields after T steps and after all of them"""
    h = _handle(rng_mode)
    out = (h.new_obs(), np.zeros(N, np.float32), np.zeros(N, np.uint8))
    for t in range(T):
        h.step(actions[t], out=out)
    first = _fields(h)
    for t in range(T, T + T2):
        h.step(actions[t], out=out)
    second = _fields(h)
    h.close()
    return first, second


def _same(got, want, what):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def given_actions():
    return np.random.RandomState(5).randint(4, size=(T + T2, N)).astype(np.int32)


@pytest.fixture(scope="module")
def twins(given_actions):
    """the single-step fields for the given action plane, once per RNG mode"""
    return {mode: _single_steps(mode, given_actions) for mode in (_lib.RNG_MT19937, _lib.RNG_PHILOX)}


def _check_two_calls(h, call, want, what):
    """call(T0, T1) runs steps T0 .. T1 - 1 on h"""
    call(0, T)
    first = _fields(h)
    _same(first, want[0], what + ", 260 steps")
    assert (first["n_finished"] == 1).all() and (first["last_length"] == 251).all() and (first["ep_length"] == T - 251).all()
    call(T, T + T2)
    second = _fields(h)
    _same(second, want[1], what + ", 5 more steps")
    assert np.array_equal(second["last_return"], first["last_return"]) and np.array_equal(second["last_length"], first["last_length"])
    assert (second["n_finished"] == 1).all()


@pytest.mark.parametrize("rng_mode, what", [(_lib.RNG_MT19937, "sequential rollout, MT19937"),
                                            (_lib.RNG_PHILOX, "episode-parallel rollout, Philox")])
def test_rollout_leaves_the_single_step_episode_fields(rng_mode, what, given_actions, twins):
    h = _handle(rng_mode)
    _check_two_calls(h, lambda t0, t1: h.rollout(t1 - t0, actions=given_actions[t0:t1]), twins[rng_mode], what)
    h.close()


@pytest.mark.parametrize("family, rng_mode", [("linear", _lib.RNG_PHILOX), ("mlp", _lib.RNG_MT19937)])
def test_policy_rollout_leaves_the_single_step_episode_fields(family, rng_mode):
    """the policy picks the actions: the twin replays the recorded ones"""
    h = _handle(rng_mode)
    rs = np.random.RandomState(7)
    if family == "linear":
        w = rs.standard_normal(h.policy_shape())
        run = lambda steps: h.rollout_policy(steps, w)["actions"]
    else:
        hidden = 20
        w = rs.standard_normal((N, h.mlp_param_count(hidden))).astype(np.float32)
        run = lambda steps: h.rollout_mlp_policy(steps, w, hidden)["actions"]
    recorded = [run(T)]
    first = _fields(h)
    recorded.append(run(T2))
    second = _fields(h)
    h.close()
    actions = np.concatenate(recorded)
    assert actions.shape == (T + T2, N) and actions.min() >= 0 and actions.max() <= 3
    want = _single_steps(rng_mode, actions)
    _same(first, want[0], family + " policy rollout, 260 steps")
    _same(second, want[1], family + " policy rollout, 5 more steps")
    assert (first["n_finished"] == 1).all() and (first["last_length"] == 251).all()
    assert np.array_equal(second["last_return"], first["last_return"]) and np.array_equal(second["last_length"], first["last_length"])


def test_persistent_stepping_leaves_the_single_step_episode_fields(given_actions, twins):
    h = _handle(_lib.RNG_MT19937)
    h.set_persistent(True)
    out = (h.new_obs(), np.zeros(N, np.float32), np.zeros(N, np.uint8))

    def call(t0, t1):                      # (reading the fields afterwards parks the resident kernel: it stores them at its exit)
        for t in range(t0, t1):
            h.step(given_actions[t], out=out)

    _check_two_calls(h, call, twins[_lib.RNG_MT19937], "persistent stepping")
    h.close()
