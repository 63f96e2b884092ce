"""dmd_lambda_returns: the TD(lambda) recursion of the actor-critic loss as ONE launch (one thread per env row), BITWISE the Python
function it replaces on GPU tensors (`actor_critic._lambda_returns_torch`: the reference's expressions, ~10 + 4 T launches on (B,)
tensors).  Rows that are dead at every step, rows with `end` and `trunc` both set, zero and negative rewards; lambda == 0 and CPU
tensors keep the torch path.  The interpreter twin holds the kernel to an fp32 numpy restatement of the same operations."""
import numpy as np
import pytest
import torch

GAMMA = 0.985


def _case(t, seed=0):
    g = torch.Generator().manual_seed(seed + t)
    b = 7
    rew = torch.randint(-2, 3, (b, t), generator=g).float() * torch.rand(b, t, generator=g)
    rew[2, 0] = 0.0
    end = (torch.rand(b, t, generator=g) < 0.25).long()
    trunc = (torch.rand(b, t, generator=g) < 0.2).long()
    end[0], trunc[0] = 1, 0  # dead at every step
    end[1, t // 2] = trunc[1, t // 2] = 1  # both set
    end[3], trunc[3] = 0, 0  # alive throughout
    vb = torch.randn(b, t, generator=g) * 3
    return rew, end, trunc, vb


@pytest.mark.gpu
@pytest.mark.parametrize("t", [1, 5, 15])
def test_lambda_returns_kernel_bitwise_the_python_function_gpu(t):
    import diamond_amd as D
    from diamond_amd import actor_critic as AC
    from diamond_amd import native as nv

    rew, end, trunc, vb = (x.cuda() for x in _case(t))
    calls = []

    class Rec:
        def annotate(self, *a):
            pass

        def call(self, name, fn, args):
            calls.append(name)
            return fn(*args)

    old, nv.PROFILER = nv.PROFILER, Rec()
    try:
        got = D.compute_lambda_returns(rew, end, trunc, vb, GAMMA, 0.95)
        assert calls == ["dmd_lambda_returns"]
        got0 = D.compute_lambda_returns(rew, end, trunc, vb, GAMMA, 0.0)
        assert calls == ["dmd_lambda_returns"], "lambda == 0 keeps the torch path"
    finally:
        nv.PROFILER = old
    want = AC._lambda_returns_torch(rew, end, trunc, vb, GAMMA, 0.95)
    assert torch.equal(got, want), f"max diff {float((got - want).abs().max()):.3e}"
    assert torch.equal(got0, AC._lambda_returns_torch(rew, end, trunc, vb, GAMMA, 0.0))
    # (and the CPU evaluation of the same expressions, which the golden tests pin to the reference)
    assert torch.equal(got.cpu(), AC._lambda_returns_torch(*_case(t), GAMMA, 0.95))
    # a dead row's target is its own sign(rew): nothing flows in from the future or the bootstrap
    assert torch.equal(got[0], rew[0].sign())


@pytest.mark.parametrize("t", [1, 5, 15])
def test_lambda_returns_kernel_bitwise_fp32_numpy_interpreter(t):
    from diamond_amd import actor_critic as AC
    from tests.simt import loader as S
    from tests.simt.fence import fenced as G

    rew, end, trunc, vb = _case(t)
    b = rew.shape[0]
    r, e, tr, v = G(rew.numpy()), G(end.numpy()), G(trunc.numpy()), G(vb.numpy())
    ret = G(np.full((b, t), np.nan, dtype=np.float32))
    lam = 0.95
    S.check(S.lib().dmd_lambda_returns(S.ptr(r), S.ptr(e), S.ptr(tr), S.ptr(v), S.ptr(ret), b, t, GAMMA, 1 - lam, lam, None), "dmd_lambda_returns")
    f = np.float32
    g32, oml, l32 = f(GAMMA), f(1 - lam), f(lam)
    want = np.empty((b, t), dtype=np.float32)
    last = v[:, -1].copy()
    for i in reversed(range(t)):
        x = np.sign(r[:, i]) + ((1 - e[:, i]).astype(f) * g32) * ((1 - tr[:, i]).astype(f) * oml + tr[:, i].astype(f)) * v[:, i]
        alive = (np.minimum(e[:, i] + tr[:, i], 1) == 0).astype(f)
        want[:, i] = x + ((alive * g32) * l32) * last
        last = want[:, i]
    assert np.array(ret).tobytes() == want.tobytes()
    assert torch.equal(torch.from_numpy(np.array(ret)), AC._lambda_returns_torch(rew, end, trunc, vb, GAMMA, lam))
