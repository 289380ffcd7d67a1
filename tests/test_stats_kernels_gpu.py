"""-m gpu: the phase-statistics launches (csrc/stats.hip: bmnas_phase_stats_acc / _f1) through bmnas.lib against the
numpy restatement of tests/stats_ref.py — every word exactly, the loss word bit for bit.

Every tensor sits inside a larger buffer between sentinel words, one element (`pad` 1: the logits off the 16-byte
grid, the path of the guarded element loads) or four (`pad` 4: on it) behind its start; three launches of different n
run into one accumulator; (1024, 23) spans more than one workgroup."""
import ctypes

import numpy as np
import pytest
import torch

import stats_ref as R
from gpu_util import dev

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (3, 5), (7, 23), (64, 60), (65, 83), (128, 128), (1024, 23)]
F_SENT, I_SENT = 1234.5, -0x0123456789ABCDE
E_ARG = -1


def _lib():
    from bmnas import lib
    return lib


class Framed:
    """A tensor inside a buffer of sentinels: `pad` of them in front, eight behind."""

    def __init__(self, host, pad):
        host = np.ascontiguousarray(host)
        sent = I_SENT if host.dtype == np.int64 else F_SENT
        self.sent, self.pad, self.size = sent, pad, host.size
        buf = np.full(pad + host.size + 8, sent, dtype=host.dtype)
        buf[pad:pad + host.size] = host.reshape(-1)
        self.buf = torch.from_numpy(buf).to(dev())
        self.t = self.buf[pad:pad + host.size].view(host.shape)
        self.want = host.copy()

    def intact(self):
        """sentinels untouched — and, for an input, the tensor itself"""
        b = self.buf.cpu().numpy()
        return bool((b[:self.pad] == self.sent).all() and (b[self.pad + self.size:] == self.sent).all())

    def unchanged(self):
        return self.intact() and self.t.cpu().numpy().tobytes() == self.want.tobytes()


def _batches(kind, n, O, seed, thr):
    rng = np.random.default_rng(seed)
    out = []
    for i, m in enumerate((n, n + 3, n + 1)):         # three launches of different n
        x = (rng.standard_normal((m, O)) * 2).astype(np.float32)
        loss = np.float32(rng.random() * 3)
        if kind == 'acc':
            y = rng.integers(0, O, m).astype(np.int64)
            hit = rng.random(m) < 0.5                 # half the labels ARE the argmax
            y[hit] = np.array([R.argmax_first(r) for r in x])[hit]
        else:
            x = R.off_band(x, thr)
            y = (rng.random((m, O)) < 0.4).astype(np.float32)
        out.append((x, y, None if i == 1 else loss))  # the second launch has no loss term (NULL)
    return out


@pytest.mark.parametrize('pad', [1, 4])
@pytest.mark.parametrize('n,O', SHAPES)
@pytest.mark.parametrize('kind', ['acc', 'f1'])
def test_three_launches_into_one_accumulator(kind, n, O, pad):
    lib = _lib()
    assert lib.phase_stats_words(O) == R.words(O) == 4 + 3 * O
    thr = R.logit_threshold(0.3)
    want = R.empty(O)
    acc = Framed(R.empty(O), 1)
    for x, y, loss in _batches(kind, n, O, 100 * n + O, thr):
        fx, fy = Framed(x, pad), Framed(y, pad if kind == 'f1' else 1)
        floss = None if loss is None else Framed(np.array([loss], dtype=np.float32), 3)
        tl = None if loss is None else floss.t.view(())
        if kind == 'acc':
            lib.phase_stats_acc(fx.t, fy.t, tl, acc.t)
            R.tally_acc(want, x, y, None if loss is None else float(loss))
        else:
            lib.phase_stats_f1(fx.t, fy.t, tl, thr, acc.t)
            R.tally_f1(want, x, y, None if loss is None else float(loss), thr)
        torch.cuda.synchronize()
        assert fx.unchanged() and fy.unchanged() and (floss is None or floss.unchanged())
    got = acc.t.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (got[:8], want[:8])       # every word; word 0 bit for bit
    assert acc.intact()
    assert int(got[1]) == 3 and int(got[2]) == 3 * n + 4


def test_argmax_edges():
    """first-maximum ties, a row of equal logits, NaN and +-inf logits, -0 / +0, labels -100 and O"""
    from test_stats_ref import _acc_cases
    lib = _lib()
    x, y = _acc_cases()[-1]
    y = y.astype(np.int64)
    assert -100 in y and x.shape[1] in y
    for pad in (1, 2, 3, 4):
        fx, fy, acc = Framed(x, pad), Framed(y, 1), Framed(R.empty(x.shape[1]), 1)
        lib.phase_stats_acc(fx.t, fy.t, None, acc.t)
        want = R.tally_acc(R.empty(x.shape[1]), x, y, None)
        assert int(want[3]) == int((torch.from_numpy(x).argmax(1) == torch.from_numpy(y)).sum()) > 0
        assert acc.t.cpu().numpy().tobytes() == want.tobytes() and acc.intact()
    # every sample a hit, every class in turn the (duplicated, first-wins) maximum
    O = 83
    x = np.zeros((O, O), dtype=np.float32)
    for r in range(O):
        x[r, r:] = 1.0
    fx, fy, acc = Framed(x, 1), Framed(np.arange(O, dtype=np.int64), 1), Framed(R.empty(O), 1)
    lib.phase_stats_acc(fx.t, fy.t, None, acc.t)
    assert int(acc.t[3]) == O


def test_f1_edges():
    """a logit exactly equal to the threshold is not positive; NaN is not; +-inf; a target of exactly 0.5 is not true"""
    lib = _lib()
    thr = R.logit_threshold(0.3)
    t32 = np.float32(thr)
    x = np.array([[t32, np.nextafter(t32, np.float32(9)), np.nextafter(t32, np.float32(-9)), np.nan, np.inf],
                  [-np.inf, t32, np.nan, 5.0, -5.0],
                  [t32, t32, 1.0, 1.0, np.inf]], dtype=np.float32)
    y = np.array([[1, 1, 1, 1, 0], [1, 0, 0.5, 0.5, 0.75], [0, 1, 0.5, 1, 1]], dtype=np.float32)
    for pad, pad_y in ((1, 1), (4, 4), (4, 2)):       # (4, 2): logits on the 16-byte grid, targets off it
        fx, fy, acc = Framed(x, pad), Framed(y, pad_y), Framed(R.empty(5), 1)
        lib.phase_stats_f1(fx.t, fy.t, None, thr, acc.t)
        want = R.tally_f1(R.empty(5), x, y, None, thr)
        assert acc.t.cpu().numpy().tobytes() == want.tobytes() and acc.intact() and fx.unchanged() and fy.unchanged()
    counts = want[R.HEAD:].reshape(5, 3)
    assert counts[0].tolist() == [0, 0, 2]            # column 0: thr, -inf, thr -> never positive
    assert counts[1].tolist() == [1, 0, 1]            # the next float above thr is positive, thr itself is not
    assert counts[4].tolist() == [1, 1, 1]


def test_refusals_launch_nothing():
    lib = _lib()
    so = lib.load()
    O, n = 5, 4
    x = torch.randn(n, O, device=dev())
    y = torch.zeros(n, dtype=torch.int64, device=dev())
    t = torch.zeros(n, O, device=dev())
    loss = torch.ones((), device=dev())
    acc = torch.arange(R.words(O), dtype=torch.int64, device=dev())
    keep = acc.clone()
    P = lambda v: ctypes.c_void_p(v.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad_acc = [(P(x), P(y), P(loss), n, 0, P(acc), s), (P(x), P(y), P(loss), n, 129, P(acc), s),
               (P(x), P(y), P(loss), 0, O, P(acc), s), (None, P(y), P(loss), n, O, P(acc), s),
               (P(x), None, P(loss), n, O, P(acc), s), (P(x), P(y), P(loss), n, O, None, s),
               (P(x), P(y), P(loss), n, -1, P(acc), s), (P(x), P(y), P(loss), -3, O, P(acc), s)]
    for a in bad_acc:
        assert so.bmnas_phase_stats_acc(*a) == E_ARG, a
    th = ctypes.c_float(0.0)
    bad_f1 = [(P(x), P(t), P(loss), th, n, 0, P(acc), s), (P(x), P(t), P(loss), th, n, 129, P(acc), s),
              (P(x), P(t), P(loss), th, 0, O, P(acc), s), (None, P(t), P(loss), th, n, O, P(acc), s),
              (P(x), None, P(loss), th, n, O, P(acc), s), (P(x), P(t), P(loss), th, n, O, None, s)]
    for a in bad_f1:
        assert so.bmnas_phase_stats_f1(*a) == E_ARG, a
    assert so.bmnas_phase_stats_words(0) == E_ARG and so.bmnas_phase_stats_words(128) == 388
    torch.cuda.synchronize()
    assert torch.equal(acc, keep)
    # the wrappers refuse what the launch does not take, before any launch
    with pytest.raises(lib.BmnasError):
        lib.phase_stats_acc(x, y.int(), loss, acc)
    with pytest.raises(lib.BmnasError):
        lib.phase_stats_f1(x, t[:, :4], loss, 0.0, acc)
    with pytest.raises(lib.BmnasError):
        lib.phase_stats_acc(x, y, loss, acc[:5])
    with pytest.raises(lib.BmnasError):
        lib.phase_stats_acc(torch.zeros(2, 129, device=dev()), y[:2], loss, torch.zeros(400, dtype=torch.int64,
                                                                                       device=dev()))
    torch.cuda.synchronize()
    assert torch.equal(acc, keep)


@pytest.mark.parametrize('kind', ['acc', 'f1'])
def test_two_runs_are_bit_equal(kind):
    lib = _lib()
    thr = R.logit_threshold(0.3)
    runs = []
    for _ in range(2):
        acc = torch.zeros(R.words(23), dtype=torch.int64, device=dev())
        for x, y, loss in _batches(kind, 1024, 23, 7, thr):
            tx, ty = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
            tl = None if loss is None else torch.tensor(float(loss), device=dev())
            if kind == 'acc':
                lib.phase_stats_acc(tx, ty, tl, acc)
            else:
                lib.phase_stats_f1(tx, ty, tl, thr, acc)
        runs.append(acc.cpu().numpy().tobytes())
    assert runs[0] == runs[1]


@pytest.mark.parametrize('kind', ['acc', 'f1'])
def test_launch_inside_a_captured_graph(kind):
    """Replayed three times with the static inputs rewritten between replays = three eager tallies."""
    lib = _lib()
    n, O = 64, 60
    thr = R.logit_threshold(0.3)
    batches = [(x[:n], y[:n], np.float32(0.5 + i)) for i, (x, y, _) in enumerate(_batches(kind, n, O, 21, thr))]
    sx = torch.zeros(n, O, device=dev())
    sy = torch.zeros(n, dtype=torch.int64, device=dev()) if kind == 'acc' else torch.zeros(n, O, device=dev())
    sl = torch.zeros((), device=dev())
    acc = torch.zeros(R.words(O), dtype=torch.int64, device=dev())

    def launch(target):
        if kind == 'acc':
            lib.phase_stats_acc(sx, sy, sl, target)
        else:
            lib.phase_stats_f1(sx, sy, sl, thr, target)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(acc)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(acc)
    acc.zero_()                                       # (the warm-up's tally; the capture itself ran nothing)
    eager = torch.zeros_like(acc)
    want = R.empty(O)
    for x, y, loss in batches:
        sx.copy_(torch.from_numpy(x))
        sy.copy_(torch.from_numpy(y))
        sl.fill_(float(loss))
        graph.replay()
        launch(eager)
        (R.tally_acc(want, x, y, float(loss)) if kind == 'acc' else R.tally_f1(want, x, y, float(loss), thr))
    torch.cuda.synchronize()
    assert acc.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes() == want.tobytes()
    assert int(acc[1]) == 3 and int(acc[2]) == 3 * n
