"""rtw_png_device / rtw_png_rgb8_device check their arguments before any device call."""
import raytracing_in_a_weekend_rust_amd._capi as capi


def test_png_argument_errors_need_no_device():
    lib = capi.lib
    assert lib.rtw_png_rgb8_device(0, None, 0, 4, -1, None, None, 0) == -2  # RTW_E_EMPTY_IMAGE
    assert lib.rtw_png_device(0, None, 0, 4, 0, -1, None, None, 0) == -2
    assert lib.rtw_png_rgb8_device(0, None, 4, 4, 3, None, None, 0) == -1  # RTW_E_ARG: filter outside -1..2
    assert lib.rtw_png_device(0, None, 1, 4, 4, -2, None, None, 0) == -1
    assert b"filter" in lib.rtw_last_error()
    assert lib.rtw_png_rgb8_device(0, None, 1 << 20, 1 << 20, -1, None, None, 0) == -6  # beyond one IDAT
