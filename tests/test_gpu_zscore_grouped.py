"""The z-score over G independent groups of one tensor (pa2d_zscore_grouped_*, ops.zscore_grouped_fwd / _bwd,
functional.zscore(groups=G)) on the MI355X.

The contract is bit equality: group g's y, statistics and dx are those of the ungrouped entry points on that group's rows
alone.  Each group is also held to the per-row bounds that test_gpu_slicepredictor.py applies to the ungrouped kernels: 4 x the
worst row error of the float32 CPU restatement (slicepredictor_restatement.zscore / its autograd) against float64 on the
test's own inputs.  Outputs are made in poisoned buffers (elementwise_check.poisoned)."""
import pytest
import torch

from elementwise_check import poisoned
import slicepredictor_restatement as R
from test_gpu_sequensolver import _bounded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [      # groups, rows per group, C, pitch
    (1, 5, 12, 12), (3, 5, 12, 20), (4, 70, 256, 256), (10, 4099, 64, 64),
]


def _restated(x, dy, dtype):
    xx = x.to(dtype).clone().requires_grad_(True)
    y = R.zscore(xx)
    y.backward(dy.to(dtype))
    return y.detach(), xx.grad, xx.detach().mean(), xx.detach().std(unbiased=False)


def _check_groups(buf, dbuf, groups, rpg, C, label, backward_groups=None):
    """buf / dbuf: CPU [groups * rpg, pitch]; the first C columns are the data."""
    from transformerbasednavierstokesolver_amd import ops
    xd, dyd = buf.to(DEV)[:, :C], dbuf.to(DEV)[:, :C]
    y, stats = poisoned(ops.zscore_grouped_fwd, xd, groups)
    assert y.is_contiguous() and tuple(y.shape) == (groups * rpg, C) and tuple(stats.shape) == (groups, 2)
    assert stats.dtype == torch.float64
    dx = None
    if backward_groups is None:
        dx = poisoned(ops.zscore_grouped_bwd, dyd, y, stats)
        backward_groups = range(groups)
    for g in range(groups):
        rows = slice(g * rpg, (g + 1) * rpg)
        y1, s1 = ops.zscore_fwd(xd[rows])
        assert torch.equal(y[rows], y1) and torch.equal(stats[g], s1), f"{label} group {g}: forward bits"
        x_g, dy_g = buf[rows, :C], dbuf[rows, :C]
        if float(s1[1]) == 0.0:
            assert float(y[rows].abs().max()) == 0.0
            continue
        y64, dx64, mu64, sd64 = _restated(x_g, dy_g, torch.float64)
        y32, dx32, _, _ = _restated(x_g, dy_g, torch.float32)
        assert abs(float(stats[g, 0]) - float(mu64)) <= 1e-12 * max(1.0, abs(float(mu64)))
        assert abs(float(stats[g, 1]) - float(sd64)) <= 1e-9 * float(sd64)
        _bounded("y", y[rows], y64, y32, f"{label} group {g}")
        if dx is not None and g in backward_groups:
            dx1 = ops.zscore_bwd(dyd[rows], y1, s1)
            assert torch.equal(dx[rows], dx1), f"{label} group {g}: backward bits"
            _bounded("dx", dx[rows], dx64, dx32, f"{label} group {g}")
    return y, stats, dx


@pytest.mark.parametrize("groups,rpg,C,pitch", CASES)
def test_every_group_equals_the_ungrouped_call_on_its_rows(groups, rpg, C, pitch):
    from transformerbasednavierstokesolver_amd import functional as Fn
    g = torch.Generator().manual_seed(9000 + groups + rpg + C + pitch)
    buf = torch.randn(groups * rpg, pitch, generator=g) * 0.7
    buf += torch.arange(groups).repeat_interleave(rpg).reshape(-1, 1) * 0.3      # every group its own mean ...
    buf *= (1.0 + torch.arange(groups).repeat_interleave(rpg).reshape(-1, 1))    # ... and its own scale
    dbuf = torch.randn(groups * rpg, pitch, generator=g)
    label = f"zscore_grouped groups={groups} rows={rpg} C={C} pitch={pitch}"
    y, stats, dx = _check_groups(buf, dbuf, groups, rpg, C, label)
    # the autograd node, on [groups, rpg, C]: the same bits as the two ops, and groups = 1 is the whole-tensor node
    xa = buf.to(DEV)[:, :C].reshape(groups, rpg, C).clone().requires_grad_(True)
    ya = Fn.zscore(xa, groups=groups)
    ya.backward(dbuf.to(DEV)[:, :C].reshape(groups, rpg, C))
    assert torch.equal(ya.detach().reshape(-1, C), y) and torch.equal(xa.grad.reshape(-1, C), dx)
    if groups == 1:
        xb = xa.detach().clone().requires_grad_(True)
        yb = Fn.zscore(xb)
        yb.backward(dbuf.to(DEV)[:, :C].reshape(groups, rpg, C))
        assert torch.equal(yb, ya) and torch.equal(xb.grad, xa.grad)


def test_offset_constant_and_scaled_groups_side_by_side():
    """Five groups of 257 x 64: unit, mean = 100 std, constant (exact zeros, sigma = 0), scaled by 2^40, unit.  A group's
    result must not see its neighbours.  sigma = 0 is outside the backward's contract, so the backward runs without the
    constant group."""
    rpg, C = 257, 64
    g = torch.Generator().manual_seed(9100)
    parts = [torch.randn(rpg, C, generator=g) * 0.7 for _ in range(5)]
    parts[1] = parts[1] + 70.0
    parts[2] = torch.full((rpg, C), 3.14159)
    parts[3] = parts[3] * 2.0 ** 40
    dbuf = torch.randn(5 * rpg, C, generator=g)
    y, stats, _ = _check_groups(torch.cat(parts), dbuf, 5, rpg, C, "zscore_grouped special", backward_groups=())
    assert float(stats[2, 1]) == 0.0 and float(stats[2, 0]) == float(torch.tensor(3.14159))
    assert float(y[2 * rpg:3 * rpg].abs().max()) == 0.0
    keep = [0, 1, 3, 4]
    rows = torch.cat([torch.arange(k * rpg, (k + 1) * rpg) for k in keep])
    _check_groups(torch.cat([parts[k] for k in keep]), dbuf[rows], 4, rpg, C, "zscore_grouped special, no constant group")


def test_gradient_of_the_node_against_autograd_of_the_restatement():
    """functional.zscore(x, groups=3) on [6, 7, 8] inside a small graph: the gradient that reaches the leaf against float64
    autograd of the restatement applied to the three groups."""
    from transformerbasednavierstokesolver_amd import functional as Fn
    g = torch.Generator().manual_seed(9200)
    x = torch.randn(6, 7, 8, generator=g)
    w = torch.randn(6, 7, 8, generator=g)

    def restated(dtype):
        xx = x.to(dtype).clone().requires_grad_(True)
        y = torch.cat([R.zscore(xx[2 * k:2 * k + 2] * 1.5) for k in range(3)])
        (y * w.to(dtype)).sum().backward()
        return y.detach(), xx.grad

    y64, dx64 = restated(torch.float64)
    y32, dx32 = restated(torch.float32)
    xa = x.to(DEV).requires_grad_(True)
    ya = Fn.zscore(xa * 1.5, groups=3)
    (ya * w.to(DEV)).sum().backward()
    _bounded("y", ya.detach(), y64, y32, "zscore node groups=3")
    _bounded("dx", xa.grad, dx64, dx32, "zscore node groups=3")
    # not the whole-tensor z-score: the groups have their own statistics
    assert not torch.equal(Fn.zscore(xa.detach() * 1.5), ya.detach())


def test_refusals_on_the_device():
    from transformerbasednavierstokesolver_amd import ops
    with pytest.raises(RuntimeError, match="1002"):
        ops.zscore_grouped_fwd(torch.zeros(6, 6, device=DEV), 2)            # C % 4 != 0
    with pytest.raises(ValueError, match="groups"):
        ops.zscore_grouped_fwd(torch.zeros(6, 8, device=DEV), 4)
    y, stats = ops.zscore_grouped_fwd(torch.zeros(0, 8, device=DEV), 3)     # no rows: a no-op
    assert y.shape == (0, 8) and stats.shape == (3, 2)
