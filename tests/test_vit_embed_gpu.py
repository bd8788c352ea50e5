"""basd_vit_embed_bf16 (csrc/vit_embed.hip): CLS row + position embedding (+ norm_pre) in one launch (GPU box only).

Without LayerNorm the result must equal torch's cat + add on bf16 bit for bit, with LayerNorm it must equal
basd_layernorm_fwd_bf16 of that assembled tensor bit for bit: both are existing code, so no tolerance.  One fp64
per-element check with the LayerNorm bound of tests/_ln_cases.py ties the chain to the definition.  The C entry is called
directly on an output that sits between guard frames of a NaN bit pattern no kernel produces.

D % 8 == 0 makes every row pitch a multiple of 16 bytes (136 * 2 = 272), so the (2, 5, 136) case alone still takes the
16-byte path; the element path is reached through pointers that are not 16-byte aligned, which the last test adds."""
import pytest
import torch

from tests import _ln_cases as LN

pytestmark = pytest.mark.gpu

SHAPES = [(3, 16, 128), (2, 49, 768), (2, 5, 136), (1, 1, 2048)]
GUARD = 4096                     # elements in front of and behind the output
SENTINEL = LN.SENTINEL_BF16
EPS = 1e-5
BASD_ERR_SHAPE = 1


@pytest.fixture(scope="module")
def nat():
    import basd_amd._native as native
    assert torch.cuda.is_available(), "needs an MI355X"
    native.lib()
    return native


def _case(B, N, D, with_cls, outliers=False):
    g = torch.Generator().manual_seed(100_003 * B + 1009 * N + D + int(with_cls))
    T = N + int(with_cls)
    patches = torch.randn(B, N, D, generator=g)
    if outliers:                 # CLIP's outlier channels: one channel 10^3 times the spread of the others, per row
        col = torch.randint(0, D, (B, N, 1), generator=g)
        patches.scatter_(2, col, 1000.0 * (1.0 - 2.0 * torch.randint(0, 2, (B, N, 1), generator=g).float()))
    a = {"patches": patches.bfloat16(), "cls": torch.randn(D, generator=g).bfloat16() if with_cls else None,
         "pos": (0.5 * torch.randn(T, D, generator=g)).bfloat16(),
         "gamma": 1.0 + 0.5 * torch.randn(D, generator=g), "beta": 0.1 * torch.randn(D, generator=g)}
    return {k: (None if v is None else v.cuda()) for k, v in a.items()}


def _framed(n_elements, offset=0):
    buf = torch.full((GUARD + n_elements + GUARD,), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return buf, buf[GUARD + offset:GUARD + offset + n_elements]


def _embed(nat, a, layernorm, offset=0, eps=EPS):
    """the C entry on an output inside guard frames; -> [B, T, D]"""
    B, N, D = a["patches"].shape
    T = N + int(a["cls"] is not None)
    buf, out = _framed(B * T * D, offset)
    p = nat._ptr
    rc = nat.lib().basd_vit_embed_bf16(p(a["patches"]), p(a["cls"]), p(a["pos"]), p(a["gamma"] if layernorm else None),
                                       p(a["beta"] if layernorm else None), eps, B, N, D, p(out), nat._stream())
    assert rc == 0, nat.lib().basd_last_error()
    torch.cuda.synchronize()
    bits = buf.view(torch.int16)
    assert bool((bits[:GUARD + offset] == SENTINEL).all()) and bool((bits[GUARD + offset + B * T * D:] == SENTINEL).all()), \
        "written outside the output"
    assert not bool((out.view(torch.int16) == SENTINEL).any()), "an element of the output was not written"
    return out.view(B, T, D)


def _torch_assembly(a):
    x = a["patches"]
    if a["cls"] is not None:
        x = torch.cat([a["cls"].view(1, 1, -1).expand(x.shape[0], -1, -1), x], dim=1)
    return x + a["pos"]


@pytest.mark.parametrize("layernorm", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("with_cls", [True, False], ids=["cls", "nocls"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_existing_chain_bit_for_bit(nat, shape, with_cls, layernorm):
    a = _case(*shape, with_cls)
    got = _embed(nat, a, layernorm)
    want = _torch_assembly(a)
    if layernorm:
        want = nat.layernorm_fwd(want, a["gamma"], a["beta"], EPS)[0]
    assert got.shape == want.shape
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the wrapper: same entry, torch-owned output
    y = nat.vit_embed(a["patches"], a["cls"], a["pos"], *((a["gamma"], a["beta"]) if layernorm else (None, None)), eps=EPS)
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layernorm_against_fp64_with_outlier_channels(nat, shape):
    """every element of the normalised rows inside the forward bound of tests/_ln_cases.py (its eps), on rows where one
    channel is 10^3 times the spread of the others; the reference normalises the rounded sum in fp64"""
    B, N, D = shape
    a = _case(B, N, D, True, outliers=True)
    got = _embed(nat, a, True, eps=LN.EPS)
    s64 = torch.cat([a["cls"].double().view(1, 1, D).expand(B, -1, -1), a["patches"].double()], dim=1) + a["pos"].double()
    rounded = s64.bfloat16()                                     # one rounding of the exact sum: the kernel's row
    assert float(rounded[:, 1:].float().abs().amax(-1).min()) >= 900.0
    ratios = LN.forward_ratios(rounded.view(-1, D), a["gamma"], a["beta"], got.reshape(-1, D), None, None,
                               LN.depth(LN.config(D)[1]))
    print(f"vit-embed-bound {shape} y {ratios['y']:.4f}")
    assert ratios["y"] <= 1.0, ratios


@pytest.mark.parametrize("layernorm", [False, True], ids=["plain", "ln"])
def test_unaligned_pointers_take_the_element_path_with_the_same_bits(nat, layernorm):
    """patches, cls, pos and out each start 8 bytes off a 16-byte boundary"""
    a = _case(2, 5, 136, True)
    want = _embed(nat, a, layernorm)

    def shifted(t):
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
        view = buf[4:4 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 8
        return view

    b = dict(a, patches=shifted(a["patches"]), cls=shifted(a["cls"]), pos=shifted(a["pos"]))
    assert torch.equal(_embed(nat, b, layernorm, offset=4).view(torch.int16), want.view(torch.int16))
    for name in ("patches", "cls", "pos"):                       # one unaligned pointer is enough
        assert torch.equal(_embed(nat, dict(a, **{name: b[name]}), layernorm).view(torch.int16), want.view(torch.int16))


def test_unsupported_shapes_are_refused_before_the_launch(nat):
    p = nat._ptr
    z = torch.zeros(4 * 2056, dtype=torch.bfloat16, device="cuda")
    gamma = torch.ones(2056, device="cuda")
    buf, out = _framed(4 * 2056)
    for B, N, D, cls in ((1, 2, 12, z), (1, 1, 2056, z), (2, 0, 128, None), (1, 2, 0, z), (-1, 2, 128, z)):
        rc = nat.lib().basd_vit_embed_bf16(p(z), p(cls), p(z), p(gamma), p(gamma), EPS, B, N, D, p(out), nat._stream())
        assert rc == BASD_ERR_SHAPE, (B, N, D)
    # gamma without beta, and an output that overlaps the patches
    assert nat.lib().basd_vit_embed_bf16(p(z), p(z), p(z), p(gamma), None, EPS, 1, 2, 128, p(out), nat._stream()) == BASD_ERR_SHAPE
    assert nat.lib().basd_vit_embed_bf16(p(z), None, p(out), None, None, EPS, 1, 2, 128, p(z[64:]), nat._stream()) == BASD_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == SENTINEL).all()) and not bool(z.any())
    assert nat.vit_embed_supported(768) and not nat.vit_embed_supported(12) and not nat.vit_embed_supported(2056)
