"""The rgn_image_* entries validate before they launch (no GPU): a bad shape, layout, alignment or null pointer gives a negative RGN_E_* code
and a message through rgn_last_error(); the addresses here are plausible, aligned and never dereferenced."""
from regione_amd import _lib

P = 0x10000


def _msg(h):
    return h.rgn_last_error().decode()


def test_resample_validates_its_arguments():
    h = _lib.lib()
    Q = P + 0x1000
    ok = dict(src=P, in_h=8, in_w=8, dst=Q, out_h=8, out_w=4, bounds=P, weights=P, ksize=7, axis=0)

    def call(**kw):
        a = dict(ok, **kw)
        return h.rgn_image_resample_u8(a["src"], a["in_h"], a["in_w"], a["dst"], a["out_h"], a["out_w"], a["bounds"], a["weights"], a["ksize"],
                                       a["axis"], None)
    for kw in (dict(src=None), dict(dst=None), dict(bounds=None), dict(weights=None), dict(in_w=0), dict(out_w=0), dict(ksize=0),
               dict(ksize=5000)):
        assert call(**kw) == -1 and "bad argument" in _msg(h), kw
    assert call(axis=2) == -1 and "axis" in _msg(h)
    assert call(out_h=4) == -1 and "one pass changes one dimension" in _msg(h)                   # x pass with another height
    assert call(axis=1) == -1 and "one pass changes one dimension" in _msg(h)                    # y pass with another width
    assert call(dst=P) == -1 and "differ" in _msg(h)
    assert call(src=P + 4) == -1 and "aligned" in _msg(h)
    assert call(bounds=P + 4) == -1 and "aligned" in _msg(h)
    assert call(in_h=1 << 15, out_h=1 << 15, in_w=1 << 14) == -2 and "2^28" in _msg(h)


def test_layout_kernels_validate_their_arguments():
    h = _lib.lib()
    Q = P + 0x1000
    assert h.rgn_image_u8_to_nchw_bf16(None, Q, 8, 8, P, None) == -1
    assert h.rgn_image_u8_to_nchw_bf16(P, Q, 0, 8, P, None) == -1 and "bad argument" in _msg(h)
    assert h.rgn_image_u8_to_nchw_bf16(P, Q + 2, 8, 8, P, None) == -1 and "aligned" in _msg(h)
    assert h.rgn_image_u8_to_nchw_bf16(P, Q, 1 << 15, 1 << 14, P, None) == -2
    assert h.rgn_image_patchify_u8(P, 56, 30, P, Q, 0, 1176, None) == -1 and "multiples of 28" in _msg(h)
    assert h.rgn_image_patchify_u8(P, 0, 28, P, Q, 0, 1176, None) == -1
    assert h.rgn_image_patchify_u8(P, 28, 28, P, Q, 2, 1176, None) == -1 and "out_bf16" in _msg(h)
    assert h.rgn_image_patchify_u8(P, 28, 28, P, Q, 0, 1216, None) == -1 and "ldo" in _msg(h)
    assert h.rgn_image_patchify_u8(P, 28, 28, P, Q, 1, 1180, None) == -1 and "ldo" in _msg(h)
    assert h.rgn_image_patchify_u8(P, 28, 28, P, Q, 1, 1168, None) == -1 and "ldo" in _msg(h)
    assert h.rgn_image_patchify_u8(P, 28, 28, None, Q, 0, 1176, None) == -1
    assert h.rgn_image_bf16_to_u8(P, 2, 8, Q, 8, 8, None) == -1 and "layout" in _msg(h)
    assert h.rgn_image_bf16_to_u8(P, 0, 6, Q, 8, 8, None) == -1 and "multiple of 4" in _msg(h)
    assert h.rgn_image_bf16_to_u8(P, 1, 0, Q + 4, 8, 8, None) == -1 and "aligned" in _msg(h)
    assert h.rgn_image_bf16_to_u8(None, 1, 0, Q, 8, 8, None) == -1
    assert h.rgn_image_bf16_to_u8(P, 1, 0, Q, 1 << 15, 1 << 14, None) == -2
