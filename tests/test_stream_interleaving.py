"""The one-action-stream contract across every consumer, on the oracle (tests/stream_interleaving_cases.py): every sequence without the replay and
capture operations, and every sequence WITH replays through ``StandInGraph`` -- the product's host hand-over around a graph launch
(GraphedSteps._prepare_capture / _before_replay / _after_replay), driven around engine-side step(None) calls.  ADVICE r06 (medium): a replay used to
advance the stream behind the space's back, so a host draw, a sample() that drew ahead or a seed() between two replays made the second one -- and
everything after it -- leave the NumPy sampler's stream.  The GPU half (real graphs, the per-lane states) is tests/test_gpu_stream_interleaving.py."""
import pytest

import stream_interleaving_cases as sc

MODES = {"no-graphs": None, "stand-in": sc.StandInGraph}


def _harness(env_id, oracle_factory, mode, **kw):
    return sc.Harness(env_id, oracle_factory, oracle_factory, MODES[mode], **kw)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("env_id", sc.ENV_IDS)
@pytest.mark.parametrize("name", list(sc.NAMED))
def test_named_sequence(name, env_id, mode, oracle_factory):
    sc.run(_harness(env_id, oracle_factory, mode), sc.NAMED[name])


@pytest.mark.parametrize("mode", list(MODES))
def test_masked_and_weighted_draws_between_replays(mode, oracle_factory):
    sc.run(_harness("CartPole-v1", oracle_factory, mode), sc.seq7_masked)


@pytest.mark.parametrize("mode", list(MODES))
def test_through_clip_action(mode, oracle_factory):
    sc.run(_harness("Pendulum-v1", oracle_factory, mode), sc.seq10_clip_action)


@pytest.mark.parametrize("mode", list(MODES))
def test_shared_generator_cartpole(mode, oracle_factory):
    """rng="shared" (the stand-alone sampler in front of the shared-generator step): sequences 1 and 3."""
    for seq in (sc.seq1_host_draw, sc.seq3_seed):
        sc.run(_harness("CartPole-v1", oracle_factory, mode, rng="shared"), seq)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("env_id", sc.ENV_IDS)
@pytest.mark.parametrize("seed", sc.RANDOM_SEEDS)
def test_random_sequence(seed, env_id, mode, oracle_factory):
    sc.run(_harness(env_id, oracle_factory, mode, sample_output="numpy" if seed == 1 else "torch"), sc.random_sequence(seed))


@pytest.mark.parametrize("env_id", ["CartPole-v1", "Ant-v5"])
def test_back_to_back_replays_make_no_engine_call(env_id, oracle_factory):
    sc.run(_harness(env_id, oracle_factory, "stand-in"), sc.check_back_to_back_replays_call_nothing)
