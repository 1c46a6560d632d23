"""Lit frames on the host: frame.shade_lit, the host statement of the shade
(och_gpu_render_lit_views_dev), on hand-made words with the expected words
written out; och_light_check's refusals and its boundary; the bindings."""
import numpy as np
import pytest


def word(r, g, b, a=0xFF):
    return (a << 24) | (b << 16) | (g << 8) | r


def light(ort, sun_shade=96, ao_shade=24):
    return ort.Light((0.8, 0.35, 0.25), 8 * 2.0 ** -8, sun_shade, ao_shade)


def shade1(ort, w, mask, l):
    return int(ort.shade_lit(np.array([[w]], np.uint32), np.array([[mask]], np.uint8), l)[0, 0])


def test_full_weight_is_the_identity(ort):
    rng = np.random.default_rng(5)
    f = rng.integers(0, 1 << 32, (6, 7), dtype=np.uint64).astype(np.uint32)
    # no bit set: w = 256, (c * 256 + 128) >> 8 = c for every byte
    assert np.array_equal(ort.shade_lit(f, np.zeros((6, 7), np.uint8), light(ort)), f)
    # shades of 0: every mask leaves w = 256
    m = rng.integers(0, 64, (6, 7)).astype(np.uint8)
    assert np.array_equal(ort.shade_lit(f, m, light(ort, 0, 0)), f)


def test_weights_written_out(ort):
    l = light(ort)                                       # sun 96, ao 24
    # shadowed only: w = 160.  255 * 160 + 128 = 40928 -> 159;  128 * 160 + 128 = 20608 -> 80;  1 * 160 + 128 -> 1
    assert shade1(ort, word(255, 128, 1), 0x10, l) == word(159, 80, 1)
    # self-shadowed: bit 5 adds nothing beyond bit 4
    assert shade1(ort, word(255, 128, 1), 0x30, l) == word(159, 80, 1)
    # two AO rays: w = 208.  200 * 208 + 128 = 41728 -> 163;  100 * 208 + 128 = 20928 -> 81;  10 * 208 + 128 = 2208 -> 8
    assert shade1(ort, word(200, 100, 10), 0x05, l) == word(163, 81, 8)
    # everything: w = 256 - 96 - 96 = 64.  255 * 64 + 128 = 16448 -> 64;  3 * 64 + 128 = 320 -> 1;  1 * 64 + 128 -> 0
    assert shade1(ort, word(255, 3, 1), 0x1F, l) == word(64, 1, 0)


def test_the_half_rounds_up(ort):
    l = light(ort, 128, 0)                               # shadowed: w = 128, c / 2
    # 1 * 128 + 128 = 256 -> 1 (0.5 up);  3 * 128 + 128 = 512 -> 2 (1.5 up);  2 * 128 + 128 = 384 -> 1 (exact)
    assert shade1(ort, word(1, 3, 2), 0x10, l) == word(1, 2, 1)
    # just below the half stays down: w = 127 (sun 129): 1 * 127 + 128 = 255 -> 0
    assert shade1(ort, word(1, 1, 1), 0x10, light(ort, 129, 0)) == word(0, 0, 0)


def test_channels_do_not_carry_and_alpha_is_kept(ort):
    l = light(ort, 1, 0)                                 # shadowed: w = 255
    # 255 * 255 + 128 = 65153 -> 254 in every channel: the largest product; a carry would reach the next byte
    assert shade1(ort, word(255, 0, 255, 0x12), 0x10, l) == word(254, 0, 254, 0x12)
    assert shade1(ort, word(0, 255, 0, 0x00), 0x10, l) == word(0, 254, 0, 0x00)
    # w = 0 (sun 256): colour to black, alpha as it was
    assert shade1(ort, word(255, 255, 255, 0xA5), 0x10, light(ort, 256, 0)) == word(0, 0, 0, 0xA5)


def test_pixels_that_are_no_face_hit_are_untouched(ort):
    l = light(ort)
    f = np.array([[0xFFFEBF00, 0xFF07193F, word(200, 100, 10)]], np.uint32)
    m = np.array([[0x80, 0x80, 0x1F]], np.uint8)
    assert ort.shade_lit(f, m, l).tolist() == [[0xFFFEBF00, 0xFF07193F, word(50, 25, 3)]]   # w = 64: 12928 -> 50, 6528 -> 25, 768 -> 3
    with pytest.raises(ValueError):
        ort.shade_lit(f, m[:, :2], l)


def refused(ort, l):
    with pytest.raises(ort.OchError) as e:
        ort.light_check(l)
    return e.value.status == -1


def test_light_check_refusals(ort):
    SUN, AO = ort.LIGHT_SUN, ort.LIGHT_AO
    ort.light_check(light(ort))                                              # the tests' light is fine
    ort.light_check(ort.Light())                                             # no flags: nothing to check but the shades
    assert refused(ort, ort.Light((1, 0, 0), 0.1, flags=4))                   # unknown flags
    assert refused(ort, ort.Light((1, 0, 0), 0.1, flags=SUN | AO | 8))
    assert refused(ort, ort.Light((1, 0, 0), 0.1, flags=-1))
    assert refused(ort, ort.Light((0, 0, 0)))                                 # an all-zero sun
    assert refused(ort, ort.Light((0.0, -0.0, 0.0)))
    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in range(3):
            s = [0.5, 0.5, 0.5]
            s[k] = bad
            assert refused(ort, ort.Light(s))                                 # a non-finite sun
        assert refused(ort, ort.Light(ao_reach=bad))                          # a non-finite reach
    assert refused(ort, ort.Light(ao_reach=0.0))
    assert refused(ort, ort.Light(ao_reach=-1.0))
    # the same values pass when their term is not requested
    ort.light_check(ort.Light((0, 0, 0), 0.1, flags=AO))
    ort.light_check(ort.Light((0, 0, 1), float("nan"), flags=SUN))
    ort.light_check(ort.Light((0, 0, 1), 2.0 ** -140))                        # a denormal reach is > 0
    assert refused(ort, ort.Light((0, 0, 1), 0.1, sun_shade=-1))              # shades out of range
    assert refused(ort, ort.Light((0, 0, 1), 0.1, sun_shade=257, ao_shade=0))
    assert refused(ort, ort.Light((0, 0, 1), 0.1, sun_shade=0, ao_shade=-1))
    assert refused(ort, ort.Light((0, 0, 1), 0.1, sun_shade=0, ao_shade=65))
    assert refused(ort, ort.Light(sun_shade=300))                             # also with no flags
    assert refused(ort, ort.Light((0, 0, 1), 0.1, sun_shade=1, ao_shade=64))  # 1 + 256 > 256
    assert refused(ort, ort.Light((0, 0, 1), 0.1, sun_shade=253, ao_shade=1))
    with pytest.raises(ort.OchError):
        ort._lib.call("och_light_check", None)


def test_light_check_accepts_the_boundary(ort):
    for sun, ao in ((256, 0), (0, 64), (252, 1), (128, 32), (96, 40)):
        assert sun + 4 * ao == 256
        ort.light_check(ort.Light((0, 0, 1), 0.1, sun_shade=sun, ao_shade=ao))
    ort.light_check(ort.Light((0, 0, 1), 0.1, sun_shade=0, ao_shade=0))


def test_new_symbols_are_bound(ort):
    import ctypes as C
    for name in ("och_light_check", "och_gpu_render_lit_views_dev", "och_gpu_render_lit_masks_views_dev",
                 "och_gpu_render_lit"):
        assert name in ort._lib.PROTOTYPES and hasattr(ort.load(), name)
    assert C.sizeof(ort.Light) == 28                     # 3 + 1 floats, 3 int32
    l = ort.Light((0.8, 0.35, 0.25), 0.5)
    assert l.flags == ort.LIGHT_SUN | ort.LIGHT_AO and (l.sun_shade, l.ao_shade) == (96, 24)
    for name in ("render_lit", "render_lit_views_dev", "render_lit_masks_views_dev"):
        assert callable(getattr(ort.GpuPool, name))
