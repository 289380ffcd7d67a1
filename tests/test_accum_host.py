"""CPU: the host side of gradient accumulation — `_loop.accum_steps` (parsing and clamping of args.accum_steps), the weight
rule of bmnas.optim.accum_weights for reduction 'mean' / 'sum', and the three combinations `_loop.run` refuses at its
start, before it touches the model or a GPU."""
import types

import pytest

import models.search.train_searchable._loop as loop
from bmnas import lib, optim


def _args(**kw):
    return types.SimpleNamespace(**kw)


def test_accum_steps_parsing_and_clamping(monkeypatch):
    monkeypatch.delenv('BMNAS_STEPS_PER_REPLAY', raising=False)
    assert lib.accum_max() == 8
    assert loop.accum_steps(_args()) == 1                       # absent: the loop does what it does now
    assert loop.accum_steps(_args(accum_steps=None)) == 1
    assert loop.accum_steps(_args(accum_steps=1)) == 1
    assert loop.accum_steps(_args(accum_steps=3)) == 3
    assert loop.accum_steps(_args(accum_steps='4')) == 4        # argparse without type=int
    assert loop.accum_steps(_args(accum_steps=8)) == 8
    assert loop.accum_steps(_args(accum_steps=96)) == lib.accum_max()
    assert loop.accum_steps(_args(accum_steps=0)) == 1 and loop.accum_steps(_args(accum_steps=-2)) == 1
    assert loop.accum_steps(_args(accum_steps='many')) == 1


def test_weight_rule_for_mean_and_sum():
    assert optim.accum_weights([4, 4], 'mean') == [0.5, 0.5]
    assert optim.accum_weights([5, 3], 'mean') == [5 / 8, 3 / 8]
    ws = optim.accum_weights([8, 8, 4], 'mean')
    assert ws == [0.4, 0.4, 0.2] and abs(sum(ws) - 1.0) < 1e-15
    assert optim.accum_weights([7], 'mean') == [1.0]            # one batch: the bits of its gradient
    assert optim.accum_weights([5, 3], 'sum') == [1.0, 1.0]
    assert optim.accum_weights([5, 3]) == [5 / 8, 3 / 8]        # default: mean
    for bad in ([], [4, 0], [-1, 3]):
        with pytest.raises(lib.BmnasError, match='positive'):
            optim.accum_weights(bad, 'mean')
    with pytest.raises(lib.BmnasError, match="'mean' or 'sum'"):
        optim.accum_weights([4, 4], 'none')


def test_refused_combinations(monkeypatch):
    monkeypatch.delenv('BMNAS_STEPS_PER_REPLAY', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert loop.check_accum(_args()) == 1
    assert loop.check_accum(_args(accum_steps=2)) == 2
    # without accumulation each of the three stays allowed
    assert loop.check_accum(_args(steps_per_replay=4, unrolled=True), world=2) == 1
    with pytest.raises(ValueError, match='steps_per_replay'):
        loop.check_accum(_args(accum_steps=2, steps_per_replay=2))
    with pytest.raises(ValueError, match='unrolled'):
        loop.check_accum(_args(accum_steps=2, unrolled=True))
    with pytest.raises(ValueError, match='data parallelism'):
        loop.check_accum(_args(accum_steps=2), world=2)
    monkeypatch.setenv('BMNAS_STEPS_PER_REPLAY', '2')           # the environment's k counts too
    with pytest.raises(ValueError, match='steps_per_replay'):
        loop.check_accum(_args(accum_steps=2))


@pytest.mark.parametrize('extra,match', [(dict(steps_per_replay=2), 'steps_per_replay'), (dict(unrolled=True), 'unrolled')])
def test_run_refuses_at_its_start(extra, match, monkeypatch):
    monkeypatch.delenv('BMNAS_STEPS_PER_REPLAY', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    # nothing else is looked at: no model, no loaders
    with pytest.raises(ValueError, match=match):
        loop.run(None, None, None, None, None, None, None, None, 1, None, None, _args(accum_steps=2, **extra), 'eval',
                 None, None, None, None)


def test_run_refuses_more_than_one_rank(monkeypatch):
    monkeypatch.delenv('BMNAS_STEPS_PER_REPLAY', raising=False)
    monkeypatch.setattr(loop, '_world', lambda: 2)
    with pytest.raises(ValueError, match='data parallelism'):
        loop.run(None, None, None, None, None, None, None, None, 1, None, None, _args(accum_steps=4), 'eval',
                 None, None, None, None)
