"""ops.attention_wide on the CPU is the fp32 reference of ops.attention."""
import torch

from sdwd_amd import ops


def test_cpu_matches_attention():
    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, 1, 37, 256, generator=g)
    k = torch.randn(2, 1, 45, 256, generator=g)
    v = torch.randn(2, 1, 45, 256, generator=g)
    assert not ops.attention_wide_supported(q, k, v)
    assert torch.equal(ops.attention_wide(q, k, v), ops.attention(q, k, v))
    assert torch.equal(ops.attention_wide(q, k, v, 0.25),
                       ops.attention(q, k, v, 0.25))
