"""float64 statement of a SEQUENCE of training-mode BatchNorm calls under nn.BatchNorm1d's momentum rule, for
tests/test_bn_momentum_gpu.py (the HIP finalisers against it) and tests/test_bn_momentum_ref.py (this file against
torch.nn.BatchNorm1d in float64 on the CPU).  Nothing of the product is imported: tensors in, tensors out.

    momentum m (a float):  running = (1 - m) running + m batch
    momentum None:         num_batches_tracked += 1 first, then m = 1 / num_batches_tracked   (cumulative average)

batch = the batch mean, and the UNBIASED batch variance (N / (N - 1) of the biased one the output is normalised with);
the counter is incremented by every training-mode call whatever the momentum.
"""
import torch

EPS = 1e-5


def factor(momentum, nbt_before):
    """The factor one call applies: momentum, or 1 / (counter after this call's increment) for None."""
    return 1.0 / (int(nbt_before) + 1) if momentum is None else float(momentum)


def batch_stats(x):
    """x (b, M, L) -> (mean, biased variance, unbiased variance) per channel, float64, N = b L"""
    x = x.double()
    N = x.shape[0] * x.shape[2]
    mean = x.mean(dim=(0, 2))
    var = ((x - mean[None, :, None]) ** 2).mean(dim=(0, 2))
    return mean, var, var * N / (N - 1)


def update(rm, rv, nbt, mean, unbiased, momentum):
    """One call's update of (running_mean, running_var, num_batches_tracked) from the batch statistics -> new triple."""
    f = factor(momentum, nbt)
    return (1.0 - f) * rm.double() + f * mean.double(), (1.0 - f) * rv.double() + f * unbiased.double(), int(nbt) + 1


def bn_sequence(xs, bn_w, bn_b, rm, rv, nbt, momentum):
    """Training-mode BatchNorm over the batches xs in turn -> (outputs, running_mean, running_var, counter).
    output = (x - mean) / sqrt(biased var + eps) * bn_w + bn_b."""
    rm, rv, nbt = rm.double().clone(), rv.double().clone(), int(nbt)
    outs = []
    for x in xs:
        mean, var, unbiased = batch_stats(x)
        outs.append((x.double() - mean[None, :, None]) / torch.sqrt(var + EPS)[None, :, None]
                    * bn_w.double()[None, :, None] + bn_b.double()[None, :, None])
        rm, rv, nbt = update(rm, rv, nbt, mean, unbiased, momentum)
    return outs, rm, rv, nbt
