"""CPU: the closed-form GeM backward that csrc/resnet.hip implements (tests/gem_head_oracle.py) equals fp64 autograd of the
reference's formula, and positions at or below eps get exactly zero gradient."""
import pytest
import torch

import gem_head_oracle as G


@pytest.mark.parametrize("p", [3.0, 2.3])
@pytest.mark.parametrize("HW,C", [(5, 64), (84, 64)])
def test_closed_form_equals_autograd(HW, C, p):
    x = G.make_rows(3, HW, C, seed=HW + C, bf16=False).double()
    dy = torch.randn(3, C, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    ref = G.autograd_reference(x, p, dy, torch.float64)
    dx, dp = G.gem_backward_closed_form(x, torch.tensor(p, dtype=torch.float64), dy)
    assert float((dx - ref["dx"]).abs().max()) <= 1e-13 * max(1.0, float(ref["dx"].abs().max()))
    assert abs(float(dp) - float(ref["dp"])) <= 1e-11 * max(1.0, abs(float(ref["dp"])))
    dead = x <= G.EPS
    assert bool(dead.any()) and bool((x < 0).any()) and float(ref["dx"][dead].abs().max()) == 0.0 and float(dx[dead].abs().max()) == 0.0


def test_head_train_exists_and_refuses_cpu_rows():
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    model = ResNetIBN()
    with pytest.raises(NotImplementedError):
        model.head_train(torch.zeros(10, 1024), 2, 5)
