"""-m gpu: the one-action-stream contract across replays of real HIP graphs of the random policy (tests/stream_interleaving_cases.py;
HipVectorEnv.capture_steps(policy="random")).  ADVICE r06 (medium): besides the host half that tests/test_stream_interleaving.py pins on the oracle, the
captured kernels read the per-lane states of the stream on the device -- which ``action_space.seed()``, a returned draw-ahead (mi_action_skip) and a rollout
of a kind that does not keep them (MuJoCo) leave behind, so that a later replay re-issued draws that were already consumed."""
import pytest

import stream_interleaving_cases as sc

pytestmark = pytest.mark.gpu


def _harness(env_id, oracle_factory, **kw):
    return sc.Harness(env_id, None, oracle_factory, sc.gpu_graph, **kw)


@pytest.mark.parametrize("env_id", sc.ENV_IDS)
@pytest.mark.parametrize("name", list(sc.NAMED))
def test_named_sequence(name, env_id, oracle_factory):
    sc.run(_harness(env_id, oracle_factory), sc.NAMED[name])


def test_masked_and_weighted_draws_between_replays(oracle_factory):
    sc.run(_harness("CartPole-v1", oracle_factory), sc.seq7_masked)


def test_through_clip_action(oracle_factory):
    sc.run(_harness("Pendulum-v1", oracle_factory), sc.seq10_clip_action)


def test_shared_generator_cartpole(oracle_factory):
    """rng="shared" (the stand-alone sampler in front of the shared-generator step) is capturable: sequences 1 and 3."""
    for seq in (sc.seq1_host_draw, sc.seq3_seed):
        sc.run(_harness("CartPole-v1", oracle_factory, rng="shared"), seq)


@pytest.mark.parametrize("env_id", sc.ENV_IDS)
@pytest.mark.parametrize("seed", sc.RANDOM_SEEDS)
def test_random_sequence(seed, env_id, oracle_factory):
    sc.run(_harness(env_id, oracle_factory, sample_output="numpy" if seed == 1 else "torch"), sc.random_sequence(seed))


@pytest.mark.parametrize("env_id", ["CartPole-v1", "Ant-v5"])
def test_back_to_back_replays_make_no_engine_call(env_id, oracle_factory):
    sc.run(_harness(env_id, oracle_factory), sc.check_back_to_back_replays_call_nothing)
