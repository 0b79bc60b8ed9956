"""The reference the shadow tests compare the kernels with (tests/helpers.py bf16_bits / bf16_value: plain numpy integer
arithmetic, the definition documented in csrc/dsea_device.h) pinned bit for bit against torch's own fp64 -> fp32 -> bf16
conversion.  No GPU, no library call."""
import numpy as np
import torch

from helpers import bf16_bits, bf16_chosen_values, bf16_value


def torch_bits(x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return t.float().to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_bf16_bits_equals_torch_on_normal_draws_across_40_binades():
    rng = np.random.RandomState(20240)
    x = rng.randn(100000) * np.exp2(rng.randint(-20, 20, size=100000).astype(np.float64))
    assert np.unique(np.frexp(x)[1]).size >= 40
    assert np.array_equal(bf16_bits(x), torch_bits(x))


def test_bf16_bits_on_chosen_values():
    x = bf16_chosen_values()
    got = bf16_bits(x)
    assert np.array_equal(got, torch_bits(x))
    half = x.size // 2
    want = {0.0: 0x0000,
            1.0 + 2.0 ** -8: 0x3F80,                     # tie -> even neighbour (down)
            1.0 + 3.0 * 2.0 ** -8: 0x3F82,               # tie -> even neighbour (up)
            1.0 + 2.0 ** -8 + 2.0 ** -40: 0x3F80,        # the project means TWO roundings: fp32 first, then the tie to even
            float(np.nextafter(2.0, 0.0)): 0x4000,
            2.0 - 2.0 ** -23: 0x4000,
            1.0 + 2.0 ** -7 - 2.0 ** -30: 0x3F81,
            2.0 ** -149: 0x0000, 2.0 ** -134: 0x0000, 2.0 ** -133: 0x0001, 3.0 * 2.0 ** -134: 0x0002, 2.0 ** -127: 0x0040,
            1e-300: 0x0000}
    assert len(want) == half - 1                          # (1e-40 is pinned by torch only)
    for v, b in want.items():
        (idx,) = np.nonzero(x[:half] == v)
        assert idx.size == 1, v
        assert got[idx[0]] == b, (v, hex(got[idx[0]]))
        assert got[half + idx[0]] == (b | 0x8000), (v, hex(got[half + idx[0]]))      # the sign bit survives, -0 included
    # what a ONE-step rounding of 1 + 2^-8 + 2^-40 would store: the value lies above the midpoint
    assert 1.0 + 2.0 ** -8 + 2.0 ** -40 > 0.5 * (bf16_value(0x3F80)[0] + bf16_value(0x3F81)[0])


def test_bf16_value_inverts_bf16_bits():
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    finite = (bits & 0x7F80) != 0x7F80
    v = bf16_value(bits[finite])
    assert v.dtype == np.float64
    assert np.array_equal(bf16_bits(v), bits[finite])
    t = torch.from_numpy(bits[finite].view(np.int16).copy()).view(torch.bfloat16).double().numpy()
    assert np.array_equal(v, t) and np.array_equal(np.signbit(v), np.signbit(t))
    assert bf16_value(np.uint16(0x3F80))[0] == 1.0 and bf16_value(np.uint16(0xC000))[0] == -2.0
    assert np.isnan(bf16_value(np.uint16(0x7FC0))[0])    # the sentinel of the GPU tests
