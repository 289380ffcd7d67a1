"""CPU: tests/stats_ref.py — the numpy restatement the GPU tests of the phase-statistics launch compare with — pinned
against what the trainer loop computes today: torch's argmax / `==`, `torch.sigmoid(x) > th`, sklearn's f1_score
(zero_division=1) and the loop's float64 loss accumulation."""
import numpy as np
import pytest
import torch

import stats_ref as R


def _acc_cases():
    rng = np.random.default_rng(5)
    nan, inf = float('nan'), float('inf')
    cases = []
    for n, O in ((1, 2), (3, 5), (7, 23), (64, 60), (9, 128)):
        x = rng.standard_normal((n, O)).astype(np.float32)
        y = rng.integers(0, O, n)
        cases.append((x, y))
    x = rng.standard_normal((12, 7)).astype(np.float32)
    x[0, :] = 0.25                                   # a row of equal logits
    x[1, 2] = x[1, 5] = 9.0                          # duplicated maxima: the first wins
    x[2, 6] = x[2, 0] = 9.0
    x[3, 3] = nan                                    # a NaN is a maximum
    x[4, 5] = x[4, 1] = nan                          # ... and the first NaN wins
    x[5, 0], x[5, 4] = inf, nan
    x[6, :] = -inf                                   # all -inf: index 0
    x[7, 2] = x[7, 4] = inf
    x[8, 1], x[8, 2] = -0.0, 0.0
    x[8, [0, 3, 4, 5, 6]] = -1.0                     # -0 == +0: the first wins
    y = np.array([0, 2, 0, 3, 1, 4, 0, 2, 1, -100, 7, 3])          # -100 and O: never equal
    cases.append((x, y))
    return cases


def test_argmax_and_equality_follow_torch():
    for x, y in _acc_cases():
        acc = R.tally_acc(R.empty(x.shape[1]), x, y, None)
        tx, ty = torch.from_numpy(x), torch.from_numpy(np.asarray(y, dtype=np.int64))
        assert [R.argmax_first(row) for row in x] == tx.argmax(1).tolist()
        assert int(acc[3]) == int((tx.argmax(1) == ty).sum())
        assert int(acc[1]) == 1 and int(acc[2]) == x.shape[0] and int(acc[0]) == 0
        assert R.accuracy(acc, x.shape[0]) == float((tx.argmax(1) == ty).sum().double()) / x.shape[0]


@pytest.mark.parametrize('th', [0.3, 0.5, 0.05, 0.9])
def test_logit_threshold_is_sigmoid_threshold_off_the_band(th):
    rng = np.random.default_rng(int(th * 100))
    thr = R.logit_threshold(th)
    x = (rng.standard_normal((200, 23)) * 2 + thr).astype(np.float32)
    x[::7, 3] = np.float32(thr + 3e-5)               # inside the band: moved out below
    x[::5, 4] = np.float32(thr)
    x = R.off_band(x, thr)
    assert R.band_empty(x, thr)                      # a condition of the input, not a tolerance
    x[0, 0], x[1, 1], x[2, 2] = np.inf, -np.inf, np.nan
    want = (torch.sigmoid(torch.from_numpy(x)) > th).numpy()
    got = x > np.float32(thr)
    assert (got == want).all()


def _f1_case(rng, n, O, kind):
    p = rng.random()
    yt = (rng.random((n, O)) < p * rng.random(O)).astype(np.float32)
    yp = rng.random((n, O)) < rng.random() * rng.random(O)
    if kind == 'absent':
        yt[:, 0] = 0
    elif kind == 'never':
        yp[:, -1] = False
    elif kind == 'zero_labels':
        yt[:] = 0
    elif kind == 'nothing':
        yt[:] = 0
        yp[:] = False
    return yt, yp


@pytest.mark.parametrize('kind', ['random', 'absent', 'never', 'zero_labels', 'nothing'])
def test_f1_from_counts_is_sklearn_f1_score(kind):
    from sklearn.metrics import f1_score
    rng = np.random.default_rng(17)
    thr = R.logit_threshold(0.3)
    for trial in range(60):
        n, O = int(rng.integers(1, 40)), int(rng.integers(2, 24))
        yt, yp = _f1_case(rng, n, O, kind)
        logits = np.where(yp, thr + 1.0, thr - 1.0).astype(np.float32)
        acc = R.empty(O)
        cut = n // 2                                  # two tallies into one accumulator
        if cut:
            R.tally_f1(acc, logits[:cut], yt[:cut], None, thr)
        R.tally_f1(acc, logits[cut:], yt[cut:], None, thr)
        assert int(acc[2]) == n
        t = yt > 0.5
        assert (acc[R.HEAD:].reshape(O, 3) == np.stack([(t & yp).sum(0), (~t & yp).sum(0), (t & ~yp).sum(0)], 1)).all()
        for avg in ('micro', 'macro', 'weighted'):
            want = float(f1_score(yt, yp, average=avg, zero_division=1))
            assert R.f1(acc, avg) == want, (kind, trial, avg)          # exact: host float64 on both sides


def test_loss_word_holds_the_bits_of_the_loops_float64_sum():
    rng = np.random.default_rng(3)
    acc = R.empty(2)
    loss_sum = torch.zeros((), dtype=torch.float64)
    x = np.zeros((1, 2), dtype=np.float32)
    for i in range(50):
        loss = torch.tensor(float(rng.random()) * 10 ** float(rng.integers(-3, 3)), dtype=torch.float32)
        n = int(rng.integers(1, 200))
        loss_sum += loss.detach().double() * n
        R.tally_acc(acc, np.repeat(x, n, 0), np.zeros(n, dtype=np.int64), float(loss))
        assert acc[0:1].tobytes() == loss_sum.numpy().tobytes(), i
    assert R.loss_sum(acc) == float(loss_sum)
    before = acc[0]
    R.tally_acc(acc, x, np.zeros(1, dtype=np.int64), None)            # no loss: the word stays
    assert acc[0] == before and int(acc[1]) == 51
