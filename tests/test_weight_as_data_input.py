"""A weight that operators read as a data input (an imported ``x + self.param``)
gets its gradient: the executor moves the input gradients its consumers return
into the parameter's gradient, and a train step updates it."""
import pytest
import torch
import torch.nn as nn

from flexflow_train_amd.core import DataType, FFConfig, FFModel, LossType, SGDOptimizer
from flexflow_train_amd.frontends.torch_fx import PyTorchModel, copy_weights


class AddParam(nn.Module):
    def __init__(self, shape, twice):
        super().__init__()
        self.lin, self.out = nn.Linear(16, 16), nn.Linear(16, 5)
        self.b = nn.Parameter(torch.randn(shape))
        self.twice = twice

    def forward(self, x):
        h = torch.tanh(self.lin(x) + self.b)
        if self.twice:                      # a second reader of the same weight
            h = h * self.b
        return self.out(h)


def _import(shape, twice, lr):
    torch.manual_seed(3)
    net = AddParam(shape, twice).eval()
    ff = FFModel(FFConfig())
    x = ff.create_tensor([4, 6, 16], DataType.DT_FLOAT, name="x")
    pm = PyTorchModel(net)
    pm.graph = None                         # the torch.export path: parameters outside Linear become weights
    pm.torch_to_ff(ff, [x])
    ff.compile(optimizer=SGDOptimizer(ff, lr=lr), loss_type=LossType.LOSS_MEAN_SQUARED_ERROR_AVG_REDUCE)
    copy_weights(ff)
    return net, ff.executor


@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("shape", [(4, 6, 16), (1, 6, 16), (16,)])
def test_gradient_matches_torch(shape, twice):
    net, ex = _import(shape, twice, 0.0)
    g = torch.Generator().manual_seed(4)
    inp, dout = torch.randn(4, 6, 16, generator=g), torch.randn(4, 6, 5, generator=g)
    out = ex.forward({"x": inp}, training=True)
    want = net(inp)
    torch.testing.assert_close(out.float(), want, rtol=1e-5, atol=1e-5)
    ex.backward(dout)
    want.backward(dout)
    assert net.b.grad.abs().sum() > 0
    torch.testing.assert_close(ex.get_parameter_grad("b.w"), net.b.grad, rtol=1e-5, atol=1e-5)
    (kn,) = [n for n in ex.parameter_names() if n.endswith(".kernel")
             and torch.equal(ex.get_parameter(n), net.lin.weight.detach().t())]
    torch.testing.assert_close(ex.get_parameter_grad(kn), net.lin.weight.grad.t(), rtol=1e-5, atol=1e-5)
    # a second backward starts from zero again
    ex.forward({"x": inp}, training=True)
    ex.backward(dout)
    torch.testing.assert_close(ex.get_parameter_grad("b.w"), net.b.grad, rtol=1e-5, atol=1e-5)


def test_train_step_updates_the_weight():
    net, ex = _import((1, 6, 16), False, 0.5)
    g = torch.Generator().manual_seed(5)
    inp, target = torch.randn(4, 6, 16, generator=g), torch.randn(4, 6, 5, generator=g)
    before = {n: ex.get_parameter(n).clone() for n in ex.parameter_names()}
    ex.train_step({"x": inp}, target)
    moved = {n: float((ex.get_parameter(n) - before[n]).abs().max()) for n in before}
    assert all(m > 0 for m in moved.values()), moved
