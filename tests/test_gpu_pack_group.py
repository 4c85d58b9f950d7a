"""The tiled grouped weight pack is bit-identical to the stand-alone pack."""


import numpy as np


import pytest


import torch


from oracle import functional as OF, train as OT


pytestmark = pytest.mark.gpu


PREC = {torch.float16: 16, torch.bfloat16: "bf16"}


@pytest.fixture(scope="module")
def A():
    import sr_amd
    assert torch.cuda.is_available()
    sr_amd._lib.load()
    return sr_amd


RCAN_KW = dict(n_feats=64, n_resgroups=2, n_resblocks=3, reduction=16, scale_factor=2)


def test_tiled_group_pack_is_bit_identical_to_the_standalone_pack(A):
    """ops.PackGroup.refresh (srk_pack_conv_weights_group_tiled: one 16 x 64-channel tile of one parameter per block, read through
    LDS) against srk_pack_conv_weights on the same parameters: every layout a model uses -- forward / dgrad, 3x3 / 1x1 / 5x5 (the
    latter through the 16-block fallback), channel counts that are not multiples of 8, 16 or 64, the PixelShuffle permutation on a
    forward layout (models/common.py Upsampler) and on a dgrad layout (fallback), bf16 and fp16 -- bit for bit, biases included,
    after the parameters changed in place."""
    from sr_amd import ops
    torch.manual_seed(11)
    shapes = [(64, 64, 3, 0), (64, 3, 3, 0), (3, 64, 3, 0), (256, 64, 3, 2), (102, 128, 3, 0), (128, 102, 3, 0), (48, 160, 1, 0),
              (64, 320, 1, 0), (12, 3, 5, 0), (36, 64, 3, 3), (200, 72, 3, 0)]
    for dt in (torch.bfloat16, torch.float16):
        params = [(torch.nn.Parameter(torch.randn(co, ci, k, k, device="cuda") * 0.1), torch.nn.Parameter(torch.randn(co, device="cuda")), ps)
                  for (co, ci, k, ps) in shapes]
        grp = ops.PackGroup()
        with ops.forward_scope(grp):
            held = [(ops.pack_conv(w, b, dt, ps_r=ps), ops.pack_conv(w, None, dt, dgrad=True, ps_r=ps)) for (w, b, ps) in params]
        with torch.no_grad():
            for (w, b, _) in params:                              # an optimizer step: new values at the same addresses
                w.mul_(-0.7).add_(0.01)
                b.add_(0.5)
        with ops.forward_scope(grp):                              # the grouped launch refreshes every layout in place
            again = [(ops.pack_conv(w, b, dt, ps_r=ps), ops.pack_conv(w, None, dt, dgrad=True, ps_r=ps)) for (w, b, ps) in params]
        torch.cuda.synchronize()
        for (w, b, ps), (pf, pd), (qf, qd), shp in zip(params, held, again, shapes):
            assert qf.wpk.data_ptr() == pf.wpk.data_ptr() and qd.wpk.data_ptr() == pd.wpk.data_ptr(), "the group serves its own buffers"
            rf = ops.pack_conv(w.detach().clone().requires_grad_(False), b.detach().clone(), dt, ps_r=ps, cache=False)
            rd = ops.pack_conv(w.detach().clone(), None, dt, dgrad=True, ps_r=ps, cache=False)
            torch.cuda.synchronize()
            assert torch.equal(qf.wpk.view(torch.int16), rf.wpk.view(torch.int16)), ("forward", shp, dt)
            assert torch.equal(qf.bias, rf.bias), ("bias", shp, dt)
            assert torch.equal(qd.wpk.view(torch.int16), rd.wpk.view(torch.int16)), ("dgrad", shp, dt)


def _stale_token_backward_matches_a_fresh_model(A, make, lr):
    """A backward that runs after a LATER forward window of the same model (its token is stale: the group's buffers were re-packed
    since) packs the weights again, and gets what a fresh model with the same weights gets from its first forward and backward."""
    import copy
    torch.manual_seed(0)
    m = make()
    m(lr)                                                 # the first window discovers the model's packs
    m2 = make()
    m2.load_state_dict(copy.deepcopy(m.state_dict()))
    m2(lr).sum().backward()
    for p in m.parameters():
        p.grad = None
    y4 = m(lr)
    y5 = m(lr)
    y4.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(y4, y5)
    for (k, a_), b_ in zip(m2.named_parameters(), m.parameters()):
        if a_.grad is not None:
            torch.testing.assert_close(a_.grad, b_.grad, rtol=1e-5, atol=1e-6, msg=k)


def test_stale_token_conv_pair_backward(A):
    """The conv kind, on EDSR-baseline's conv_pair path (batch 16)."""
    from sr_amd import ops
    before = sum(ops.PAIR_LAUNCHES)
    _stale_token_backward_matches_a_fresh_model(
        A, lambda: A.EDSR(n_feats=64, n_resblocks=16, res_scale=0.1, scale_factor=2, precision="bf16").cuda(), torch.rand(16, 3, 24, 24).cuda())
    assert sum(ops.PAIR_LAUNCHES) > before


def test_stale_token_pointwise_pair_backward(A):
    """The pw kind: WDSR-B's fused pointwise pairs (and its 3x3 convs)."""
    _stale_token_backward_matches_a_fresh_model(
        A, lambda: A.WDSR(type="B", n_feats=128, n_resblocks=2, scale_factor=2, precision="bf16").cuda(), torch.rand(2, 3, 24, 24).cuda())
