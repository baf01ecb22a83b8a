"""The MXFP4 weight format (llm_weight_dtype = "fp4") restated on the CPU: e2m1 table, round-to-nearest-even, block scales, and the
configuration checks.  The device kernels are pinned against this restatement by tests/test_mxfp4_gpu.py."""
import pytest
import torch

from mxfp4_ref import CODE_VALUES, E2M1, block_exponent, image_bytes, quantize, rne_e2m1, unpack_image

BF16 = torch.bfloat16


def _row(vals, K=32):
    w = torch.zeros(1, K, dtype=torch.float64)
    w[0, :len(vals)] = torch.tensor(vals, dtype=torch.float64)
    return w.to(BF16)


def test_all_sixteen_codes_round_trip():
    # a block with max 6 has e = 0: every e2m1 value (both signs) is its own W'
    vals = list(E2M1) + [-v for v in E2M1]
    w = _row(vals)
    codes, e8, deq = quantize(w)
    assert e8.tolist() == [[127]]
    assert codes[0, :16].tolist() == list(range(16))
    assert torch.equal(deq[0, :16].to(torch.float64), CODE_VALUES)
    assert torch.signbit(deq[0, 8]) and deq[0, 8] == 0          # code 8 is -0


@pytest.mark.parametrize("a,want", [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0),
                                    (0.2490234375, 0.0), (0.251953125, 0.5), (2.40625, 2.0), (2.59375, 3.0), (5.03125, 6.0)])
def test_round_to_nearest_even(a, want):
    got = E2M1[int(rne_e2m1(torch.tensor([a], dtype=torch.float64))[0])]
    assert got == want
    # the same through the whole quantiser, with a 6 in the block pinning e = 0
    w = _row([6.0, a, -a])
    _, e8, deq = quantize(w)
    assert e8.tolist() == [[127]]
    assert deq[0, 1].item() == want and deq[0, 2].item() == -want


def test_negative_values_that_round_to_zero_keep_their_sign():
    codes, _, deq = quantize(_row([6.0, -0.125, 0.125, -0.0]))
    assert codes[0, 1:4].tolist() == [8, 0, 8]
    assert torch.signbit(deq[0, 1]) and not torch.signbit(deq[0, 2]) and torch.signbit(deq[0, 3])


def test_scale_edges():
    # amax exactly 6 * 2^e -> e; just above (the next bf16) -> e + 1
    for e in (-10, 0, 3):
        amax = 6.0 * 2.0 ** e
        _, e8, deq = quantize(_row([amax]))
        assert int(e8) - 127 == e and deq[0, 0].item() == amax
        above = torch.tensor([amax], dtype=BF16).view(torch.int16) + 1
        _, e8, _ = quantize(_row([above.view(BF16).item()]))
        assert int(e8) - 127 == e + 1
    # all-zero block: e = 0
    codes, e8, deq = quantize(torch.zeros(2, 64, dtype=BF16))
    assert (e8 == 127).all() and (codes == 0).all() and (deq == 0).all()
    # bf16 subnormals reach the clamp at e = -127: 2^-128 = 0.5 * 2^-127 survives, 2^-133 (the smallest subnormal) rounds to 0
    tiny = 2.0 ** -128
    codes, e8, deq = quantize(_row([tiny, -tiny, 2.0 ** -133, 2.0 ** -129 * 3]))
    assert int(e8) == 0
    assert deq[0, 0].item() == tiny and deq[0, 1].item() == -tiny and deq[0, 2].item() == 0.0
    assert deq[0, 3].item() == 2.0 ** -127      # 1.5 * 2^-128 / 2^-127 = 0.75 -> 1 (tie to the even code)
    assert block_exponent(torch.tensor([2.0 ** -133], dtype=torch.float64)).item() == -127
    # the top of the format's domain (|W| < 1.75 * 2^127: from there on a value rounds up to 4 * 2^126 = 2^128, outside bf16)
    big = 1.5 * 2.0 ** 127
    _, e8, deq = quantize(_row([big, -big]))
    assert int(e8) - 127 == 125 and deq[0, 0].item() == big and deq[0, 1].item() == -big


def test_relative_error_bound():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(64, 256, generator=g) * torch.logspace(-6, 2, 64)[:, None]).to(BF16)
    _, e8, deq = quantize(w)
    s = torch.pow(2.0, e8.to(torch.float64) - 127).repeat_interleave(32, dim=1)
    err = (w.to(torch.float64) - deq.to(torch.float64)).abs()
    # half a spacing of the e2m1 grid: the grid above 1 has relative spacing <= 1/2, below 1 a step of s / 2
    bound = torch.maximum(w.to(torch.float64).abs(), s) / 4
    assert (err <= bound).all()
    assert (err / bound).max() > 0.9        # and the bound is reached
    # no block maximum is clipped: it is within a quarter of its own value
    amax = w.to(torch.float64).abs().view(64, 8, 32).amax(-1)
    amax_q = deq.to(torch.float64).abs().view(64, 8, 32).amax(-1)
    assert ((amax - amax_q).abs() <= amax / 4).all()


def test_unpack_inverts_a_cpu_packed_image():
    # build the image on the CPU from the documented layout and check unpack_image against the codes it came from
    N, K = 40, 96
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    scales = torch.randint(0, 255, (N, K // 32), generator=g, dtype=torch.uint8)
    ntt, kt8 = (N + 15) // 16, (K + 63) // 64
    np_ = (ntt + 1) // 2
    img = torch.zeros(image_bytes(N, K), dtype=torch.uint8)
    img[np_ * kt8 * 1024:] = 127
    for n in range(N):
        t, r = divmod(n, 16)
        p, i = divmod(t, 2)
        for k in range(K):
            kt, rem = divmod(k, 64)
            h, g_, j = rem // 32, (rem % 32) // 8, k % 8
            byte = ((p * kt8 + kt) * 64 + g_ * 16 + r) * 16 + (2 * i + h) * 4 + j // 2
            img[byte] |= int(codes[n, k]) << (4 * (j % 2))
        for kb in range(K // 32):
            img[np_ * kt8 * 1024 + ((p * kt8 + kb // 2) * 16 + r) * 4 + 2 * i + kb % 2] = int(scales[n, kb])
    c, s = unpack_image(img, N, K)
    assert torch.equal(c, codes) and torch.equal(s, scales)


def test_fp4_weight_dtype_is_accepted_and_w4a8_is_not():
    from unimedvl_amd.config import UniMedVLConfig
    from unimedvl_amd.weights import LLMWeights, check_llm_dtypes
    check_llm_dtypes(UniMedVLConfig(llm_weight_dtype="fp4"))
    check_llm_dtypes(UniMedVLConfig.from_dict({"llm_weight_dtype": "fp4", "llm_act_dtype": "bf16"}))
    for bad in (dict(llm_weight_dtype="fp4", llm_act_dtype="fp8"), dict(llm_weight_dtype="int4"),
                dict(llm_weight_dtype="bf16", llm_act_dtype="fp8")):
        with pytest.raises(ValueError):
            check_llm_dtypes(UniMedVLConfig(**bad))
        with pytest.raises(ValueError):          # before any tensor is touched
            LLMWeights(UniMedVLConfig(**bad), None, "cpu")
    for ok in ("bf16", "fp8"):
        check_llm_dtypes(UniMedVLConfig(llm_weight_dtype=ok))
    check_llm_dtypes(UniMedVLConfig(llm_weight_dtype="fp8", llm_act_dtype="fp8"))
