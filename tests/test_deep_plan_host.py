"""Host-side pieces of the deep value-net plan and its oracle, checked on the CPU: where the BSDE loss's Neumann residual takes
grad_x V when tiles of the genl forward left the time loop early (plan_general_deep.neumann_points), and the oracle's
dense-concat tanh net against the package's DenseNet(activation='tanh')."""
import torch

from util_cases import make_pkg_value_net, orc, psp
from path_space_pde_solver_amd import plan_general_deep as pgd


def test_neumann_points_take_the_frozen_state_of_tiles_that_left_early():
    d, K, n_last = 3, 57, 6                                  # four tiles, the last one ragged (9 trajectories)
    g = torch.Generator().manual_seed(0)
    nexec = torch.tensor([7, 6, 2, 7], dtype=torch.int32)   # tile 1 stopped exactly at n_last, tile 2 long before
    img = torch.randn(K, d + 1, generator=g)
    img[16:48] = float("nan")                                # slots those two tiles never wrote
    XN = torch.randn(K, d, generator=g)
    tN = torch.rand(K, generator=g)
    want = img.clone()
    for k in range(K):
        if int(nexec[k // 16]) <= n_last:
            want[k, :d], want[k, d] = XN[k], tN[k]
    got = pgd.neumann_points(img, nexec, n_last, XN, tN)
    assert torch.equal(got, want)
    assert torch.isfinite(got).all()
    # every tile ran through n_last: the path slot as it is
    assert torch.equal(pgd.neumann_points(img[:16], torch.tensor([7], dtype=torch.int32), n_last, XN[:16], tN[:16]), img[:16])
    # every tile left before n_last (a later rank's tiles ran longer): the final states alone
    all_left = pgd.neumann_points(img, torch.zeros(4, dtype=torch.int32), n_last, XN, tN)
    assert torch.equal(all_left, torch.cat([XN, tN[:, None]], 1))


def test_oracle_dense_concat_tanh_equals_the_package_net():
    for d_in, arch in ((4, [20, 20, 20]), (112, [1, 17, 65]), (1, [128])):
        net = dict(kind="densenet_concat_tanh", arch=arch, seed=7)
        ref = orc.value_net(d_in, 1e-3, 42, net=net)
        pkg = make_pkg_value_net(net, d_in, 1e-3, "cpu")
        assert isinstance(pkg, psp.DenseNet) and pkg.activation == "tanh"
        direct = psp.DenseNet(d_in=d_in, d_out=1, lr=1e-3, arch=arch, seed=7, activation="tanh")
        for a, b, c in zip(ref.parameters(), pkg.parameters(), direct.parameters()):
            assert torch.equal(a, b) and torch.equal(a, c)
        x = torch.randn(33, d_in, generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            want = ref(x)
            assert torch.equal(pkg(x), want)
            # the formula the deep plan recognises and the kernels implement
            assert torch.allclose(pgd._dense_concat_forward(x, list(pkg.W), "tanh"), want, rtol=1e-6, atol=1e-7)
            # and not one of the other two activations
            assert not torch.allclose(orc.value_net(d_in, 1e-3, 42, net=dict(net, kind="densenet"))(x), want)
    assert orc.value_net(3, 1e-3, 42, net=dict(kind="densenet", arch=[5], seed=1)).activation == "relu2"
    assert orc.value_net(3, 1e-3, 42, net=dict(kind="user_tanh2", arch=[5], seed=1)).activation == "tanh2"
