"""Lp losses with the interface of the reference's `TestLoss` (utils/testloss.py): constructed as
`TestLoss(d=2, p=2, size_average=True, reduction=True)`, called as `loss(pred, target)` == `rel`.
exp_ns.py uses `size_average=False`: the batch SUM of per-sample relative errors."""
import torch


def _per_sample_norm(t, p):
    return torch.linalg.vector_norm(t.reshape(t.shape[0], -1), ord=p, dim=1)


class TestLoss(object):
    __test__ = False   # keeps pytest from collecting this class

    def __init__(self, d=2, p=2, size_average=True, reduction=True):
        if d <= 0 or p <= 0:
            raise AssertionError("d and p must be positive")
        self.d, self.p, self.size_average, self.reduction = d, p, size_average, reduction

    def _finish(self, per_sample):
        if not self.reduction:
            return per_sample
        return per_sample.mean() if self.size_average else per_sample.sum()

    def abs(self, x, y):
        """mesh-size weighted absolute error: h^(d/p) * ||x - y||_p with h = 1/(points - 1)"""
        h = 1.0 / (x.shape[1] - 1.0)
        return self._finish(h ** (self.d / self.p) * _per_sample_norm(x - y, self.p))

    def rel(self, x, y):
        """||x - y||_p / ||y||_p per sample"""
        b = x.shape[0]
        return self._finish(_per_sample_norm(x.reshape(b, -1) - y.reshape(b, -1), self.p) / _per_sample_norm(y, self.p))

    def rel_decoded(self, pred, y, normalizer=None):
        """`rel` of the DECODED prediction and target (exp_pipe.py:210-213, exp_elas.py:168-170): both go through
        `normalizer.decode` and are then subtracted.  normalizer=None: the raw `rel` (exp_airfoil, exp_plas)."""
        if normalizer is None:
            return self.rel(pred, y)
        return self.rel(normalizer.decode(pred), normalizer.decode(y))

    __call__ = rel


def _rel_decoded_fusable(pred, y, normalizer):
    """fp32 CUDA prediction and target, a target that asks for no gradient (the kernels give none to y) and no normaliser
    or one whose mean and std are one-element fp32 CUDA tensors."""
    stats = () if normalizer is None else (normalizer.mean, normalizer.std)
    ts = (pred, y) + tuple(stats)
    return (all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in ts[1:])
            and pred.is_cuda and pred.dtype == torch.float32 and pred.shape[0] == y.shape[0]
            and pred.numel() == y.numel() and all(t.numel() == 1 for t in stats))


class FusedTestLoss(TestLoss):
    """Same interface; `rel` runs on the libpa2d rel-L2 kernels for p=2 GPU tensors, `rel_decoded` on the
    decoded, strided rel-L2 kernels (functional.rel_l2_affine): the normaliser's statistics stay on the device and a
    strided target view (yy[..., t:t+1]) is read in place.  A float64 or CPU target, a target that requires a gradient
    or a normaliser that is not scalar keeps the torch path."""
    __test__ = False

    def rel_decoded(self, pred, y, normalizer=None):
        if self.p != 2 or not _rel_decoded_fusable(pred, y, normalizer):
            dec = (lambda t: t) if normalizer is None else normalizer.decode
            return TestLoss.rel(self, dec(pred), dec(y))            # torch, whatever the dtypes (not the fp32 kernels)
        from ..functional import rel_l2_affine
        mean, std = (None, None) if normalizer is None else (normalizer.mean.reshape(1), normalizer.std.reshape(1))
        return self._finish(rel_l2_affine(pred, y, mean, std))

    def rel(self, x, y):
        if self.p != 2 or not x.is_cuda:
            return super().rel(x, y)
        from ..functional import rel_l2
        return self._finish(rel_l2(x, y))

    __call__ = rel
