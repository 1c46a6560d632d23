"""Supersampled lit frames on the host (och_gpu_render_lit_ssaa_views_dev): the
new entry points are exported and bound, and the definition's order -- shade
every sample, then the box mean -- on a hand-made 4 x 4 frame with its masks,
the expected bytes worked out in the comments."""
import numpy as np


def word(r, g, b, a=0xFF):
    return (a << 24) | (b << 16) | (g << 8) | r


def test_new_symbols_are_bound(ort):
    # the C ABI gains two entry points, the device form and the host form; both are exported and bound
    for name in ("och_gpu_render_lit_ssaa_views_dev", "och_gpu_render_lit_ssaa"):
        assert name in ort._lib.PROTOTYPES and hasattr(ort.load(), name)
    for name in ("render_lit_ssaa", "render_lit_ssaa_views_dev"):
        assert callable(getattr(ort.GpuPool, name))
    # the two host definitions the frame is stated with
    assert callable(ort.shade_lit) and callable(ort.box_downsample)


def test_shade_then_mean_written_out(ort):
    l = ort.Light((0.8, 0.35, 0.25), 8 * 2.0 ** -8, 96, 24)      # w = 256 - 96 [bit 4] - 24 * popcount(bits 0..3)
    sky = 0xFFFEBF00                                             # R 0x00, G 0xBF = 191, B 0xFE = 254
    a, b = word(200, 100, 10), word(255, 128, 1)
    f = np.array([[a, a, b, b],
                  [a, a, b, sky],
                  [a, b, sky, sky],
                  [b, a, sky, sky]], np.uint32)
    m = np.array([[0x00, 0x10, 0x1F, 0x05],
                  [0x05, 0x30, 0x00, 0x80],
                  [0x10, 0x10, 0x80, 0x80],
                  [0x01, 0x03, 0x80, 0x80]], np.uint8)
    # shades of a = (200, 100, 10):
    #   w 256 (0x00): (200, 100, 10)
    #   w 160 (0x10, 0x30): 200 * 160 + 128 = 32128 -> 125;  100 * 160 + 128 = 16128 -> 63;  10 * 160 + 128 = 1728 -> 6
    #   w 208 (0x05, 0x03): 41728 -> 163;  20928 -> 81;  2208 -> 8
    # shades of b = (255, 128, 1):
    #   w 64 (0x1F): 16448 -> 64;  8320 -> 32;  192 -> 0
    #   w 208 (0x05): 255 * 208 + 128 = 53168 -> 207;  128 * 208 + 128 = 26752 -> 104;  336 -> 1
    #   w 256 (0x00): (255, 128, 1)
    #   w 160 (0x10): 40928 -> 159;  20608 -> 80;  288 -> 1
    #   w 232 (0x01): 255 * 232 + 128 = 59288 -> 231;  128 * 232 + 128 = 29824 -> 116;  360 -> 1
    lit = ort.shade_lit(f, m, l)
    assert lit.tolist() == [
        [word(200, 100, 10), word(125, 63, 6), word(64, 32, 0), word(207, 104, 1)],
        [word(163, 81, 8), word(125, 63, 6), word(255, 128, 1), sky],
        [word(125, 63, 6), word(159, 80, 1), sky, sky],
        [word(231, 116, 1), word(163, 81, 8), sky, sky]]
    # s = 2, per block (sum + 2) >> 2:
    #   top left:  R 200 + 125 + 163 + 125 = 613 -> 153;  G 100 + 63 + 81 + 63 = 307 -> 77;  B 10 + 6 + 8 + 6 = 30 -> 8
    #   top right: R 64 + 207 + 255 + 0 = 526 -> 132;  G 32 + 104 + 128 + 191 = 455 -> 114;  B 0 + 1 + 1 + 254 = 256 -> 64
    #   bottom left: R 125 + 159 + 231 + 163 = 678 -> 170;  G 63 + 80 + 116 + 81 = 340 -> 85;  B 6 + 1 + 1 + 8 = 16 -> 4
    #   bottom right: the sky
    want2 = [[word(153, 77, 8), word(132, 114, 64)], [word(170, 85, 4), sky]]
    assert ort.box_downsample(lit, 2).tolist() == want2
    # s = 4, (sum + 8) >> 4: R 613 + 526 + 678 + 0 = 1817 -> 114;  G 307 + 455 + 340 + 764 = 1866 -> 117
    #   B 30 + 256 + 16 + 1016 = 1318 -> 82
    assert ort.box_downsample(lit, 4).tolist() == [[word(114, 117, 82)]]
    # the order matters even under one mask: every sample shadowed (w 160), R = 200, 200, 200, 100.
    # Shade, then mean: 125 + 125 + 125 + 63 (100 * 160 + 128 = 16128) = 438 -> (438 + 2) >> 2 = 110;
    # mean, then shade: (700 + 2) >> 2 = 175 -> (175 * 160 + 128) >> 8 = 28128 >> 8 = 109
    g = np.array([[a, a], [a, word(100, 0, 0)]], np.uint32)
    sh = np.full((2, 2), 0x10, np.uint8)
    assert ort.box_downsample(ort.shade_lit(g, sh, l), 2)[0, 0] & 0xFF == 110
    assert ort.shade_lit(ort.box_downsample(g, 2), sh[:1, :1], l)[0, 0] & 0xFF == 109
