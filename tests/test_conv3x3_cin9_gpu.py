"""conv3x3 kernel at Cin = 9, the conv_in of a 9-channel inpaint U-Net and the
first odd Cin the kernel meets in production (Cin = 4 and multiples of 8 are
what the other suites cover): one input channel beyond an 8-channel staging
group, so seven lanes of the group's transpose must come out zero. Exact
equality on integer-valued data, as in test_conv3x3_edges_gpu.py, whose case
builder and extension call these tests share.

Run on an MI355X box: pytest tests/test_conv3x3_cin9_gpu.py -m gpu -q"""

import pytest

from test_conv3x3_edges_gpu import _assert_equal, _exact_case, _ext_conv, _gpu, _run_case, gpu_test

# (B, Cin, Cout, H, W, stride, halos)
SHAPES = [
    pytest.param(2, 9, 32, 9, 40, 1, "both", id="small-config-both-halos"),
    pytest.param(1, 9, 40, 5, 136, 1, "none", id="wide-config-no-halos"),
]
_BAND_CASE = (1, 9, 32, 24, 136, 1, "none")
_BANDS = ((0, 7), (7, 16), (16, 24))


@pytest.mark.parametrize("b,cin,cout,h,w,stride,halos", SHAPES)
def test_cin9_data_preconditions(b, cin, cout, h, w, stride, halos):
    c = _exact_case(b, cin, cout, h, w, stride, halos)
    assert c["x"].shape[1] == 9 and c["weight"].shape[1] == 9
    # every input channel, the ninth included, carries weight somewhere
    assert (c["weight"] != 0).any(dim=0).any(dim=-1).any(dim=-1).all()
    _exact_case(*_BAND_CASE)


@gpu_test
@pytest.mark.parametrize("b,cin,cout,h,w,stride,halos", SHAPES)
def test_conv3x3_cin9_exact(b, cin, cout, h, w, stride, halos):
    c = _exact_case(b, cin, cout, h, w, stride, halos)
    _assert_equal(_run_case(c), c["ref"], f"{(b, cin, cout, h, w, stride, halos)}")


@gpu_test
def test_conv3x3_cin9_exact_row_band_views():
    """The interior and both halos are adjacent-row views of one [1, 9, 24, 136]
    latent, as the sliced conv_in passes them; every band equals its rows of
    the full conv."""
    c = _exact_case(*_BAND_CASE)
    full = _gpu(c["x"])
    for h0, h1 in _BANDS:
        band = full[:, :, h0:h1]
        top = full[:, :, h0 - 1 : h0] if h0 > 0 else None
        bot = full[:, :, h1 : h1 + 1] if h1 < full.shape[2] else None
        got = _ext_conv(band, c["weight"], None, 1, top, bot)
        _assert_equal(got, c["ref"][:, :, h0:h1], f"rows {h0}:{h1}")
