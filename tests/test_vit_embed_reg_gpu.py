"""basd_vit_embed_reg_bf16 (csrc/vit_embed.hip): token assembly of a ViT with register tokens in one launch (GPU box
only): out[b, 0] = cls + pos[0], out[b, 1 + r] = reg[r] (no position row), out[b, 1 + R + n] = patches[b, n] + pos[1 + n].

Without LayerNorm the result must equal the torch composition on bf16 (tests/_dinov2_ref.py) bit for bit -- a register
row is a copy, so a negative zero in it survives.  With LayerNorm every element is compared with the fp64 LayerNorm of
the rounded rows under the forward bound of tests/_ln_cases.py, the bound tests/test_vit_embed_gpu.py uses.  R = 0 must
give the bits of basd_vit_embed_bf16.  The C entry is called directly on an output between guard frames.

Cases (B, N, R, D): (3, 16, 4, 128); (2, 5, 4, 1536), ViT-g's width, three chunks per lane; (2, 7, 1, 256), one register;
and patches / reg views that start 2 bytes off their allocation, which takes the element-access path."""
import pytest
import torch

from tests import _ln_cases as LN
from tests._dinov2_ref import embed_reg_emulation

pytestmark = pytest.mark.gpu

CASES = [(3, 16, 4, 128), (2, 5, 4, 1536), (2, 7, 1, 256)]
GUARD = 4096
SENTINEL = LN.SENTINEL_BF16
BASD_ERR_SHAPE = 1


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    return native


def _case(B, N, R, D):
    g = torch.Generator().manual_seed(100_003 * B + 1009 * N + 17 * R + D)
    reg = torch.randn(max(R, 1), D, generator=g).bfloat16()
    reg[0, 0], reg[0, 1] = -0.0, 0.0                         # both zeros must come out as they went in
    a = {"patches": torch.randn(B, N, D, generator=g).bfloat16(), "cls": torch.randn(D, generator=g).bfloat16(),
         "reg": reg[:R], "pos": (0.5 * torch.randn(1 + N, D, generator=g)).bfloat16(),
         "gamma": 1.0 + 0.5 * torch.randn(D, generator=g), "beta": 0.1 * torch.randn(D, generator=g)}
    return {k: v.cuda() for k, v in a.items()}


def _embed(nat, a, layernorm, eps=LN.EPS):
    """the C entry on an output inside guard frames; -> [B, 1 + R + N, D]"""
    B, N, D = a["patches"].shape
    R = a["reg"].shape[0]
    T = 1 + R + N
    buf = torch.full((GUARD + B * T * D + GUARD,), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    out = buf[GUARD:GUARD + B * T * D]
    p = nat._ptr
    rc = nat.lib().basd_vit_embed_reg_bf16(p(a["patches"]), p(a["cls"]), p(a["reg"]) if R else None, R, p(a["pos"]),
                                           p(a["gamma"] if layernorm else None), p(a["beta"] if layernorm else None),
                                           eps, B, N, D, p(out), nat._stream())
    assert rc == 0, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    bits = buf.view(torch.int16)
    assert bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + B * T * D:] == SENTINEL).all()), \
        "written outside the output"
    assert not bool((out.view(torch.int16) == SENTINEL).any()), "an element of the output was not written"
    return out.view(B, T, D)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_plain_assembly_is_the_torch_composition_bit_for_bit(nat, case):
    a = _case(*case)
    got = _embed(nat, a, False)
    want = embed_reg_emulation(a["patches"], a["cls"], a["reg"], a["pos"])
    assert got.shape == want.shape and torch.equal(got.view(torch.int16), want.view(torch.int16))
    R = case[2]
    assert torch.equal(got[:, 1:1 + R].view(torch.int16), a["reg"].expand(case[0], -1, -1).contiguous().view(torch.int16))
    y = nat.vit_embed(a["patches"], a["cls"], a["pos"], reg=a["reg"].view(1, R, -1))          # the wrapper
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_layernorm_against_fp64(nat, case):
    """every element of the normalised rows (register rows included) inside the forward bound of tests/_ln_cases.py;
    the reference normalises the rounded rows in fp64.  It is also bitwise the LayerNorm kernel on the assembled rows."""
    B, N, R, D = case
    a = _case(*case)
    got = _embed(nat, a, True)
    rounded = embed_reg_emulation(a["patches"], a["cls"], a["reg"], a["pos"])
    ratios = LN.forward_ratios(rounded.view(-1, D), a["gamma"], a["beta"], got.reshape(-1, D), None, None,
                               LN.depth(LN.config(D)[1]))
    print(f"vit-embed-reg-bound {case} y {ratios['y']:.4f}")
    assert ratios["y"] <= 1.0, ratios
    want = nat.layernorm_fwd(rounded, a["gamma"], a["beta"], LN.EPS)[0]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    y = nat.vit_embed(a["patches"], a["cls"], a["pos"], a["gamma"], a["beta"], LN.EPS, reg=a["reg"])
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("layernorm", [False, True], ids=["plain", "ln"])
def test_two_byte_offset_views_take_the_element_path_with_the_same_bits(nat, layernorm):
    a = _case(3, 16, 4, 128)
    want = _embed(nat, a, layernorm)

    def shifted(t):
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 2
        return view

    for name in ("patches", "reg"):
        got = _embed(nat, dict(a, **{name: shifted(a[name])}), layernorm)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), name


@pytest.mark.parametrize("layernorm", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("shape", [(3, 16, 128), (2, 5, 1536)], ids=lambda s: "x".join(map(str, s)))
def test_no_registers_is_the_existing_entry_bit_for_bit(nat, shape, layernorm):
    B, N, D = shape
    a = _case(B, N, 0, D)
    got = _embed(nat, a, layernorm)
    want = torch.empty(B, 1 + N, D, dtype=torch.bfloat16, device="cuda")
    p = nat._ptr
    rc = nat.lib().basd_vit_embed_bf16(p(a["patches"]), p(a["cls"]), p(a["pos"]), p(a["gamma"] if layernorm else None),
                                       p(a["beta"] if layernorm else None), LN.EPS, B, N, D, p(want), nat._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_registers_without_a_cls_token_are_refused(nat):
    a = _case(2, 5, 4, 128)
    out = torch.full((2 * 10 * 128,), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    p = nat._ptr
    L = nat.lib()
    for cls, reg, R in ((None, a["reg"], 4), (a["cls"], None, 4), (a["cls"], a["reg"], -1)):
        rc = L.basd_vit_embed_reg_bf16(p(a["patches"]), p(cls), p(reg), R, p(a["pos"]), None, None, LN.EPS, 2, 5, 128,
                                       p(out), nat._stream())
        assert rc == BASD_ERR_SHAPE and b"vit_embed_reg_bf16" in L.basd_last_error()
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == SENTINEL).all())
