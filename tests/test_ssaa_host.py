"""frame.box_downsample: the host statement of the supersampled frame
(och_gpu_render_ssaa_views_dev): every byte of an output word is the mean of
its s x s block's bytes, rounded half up, in integers.  Hand-made blocks with
their expected words written out, then a second computation on a random frame."""
import numpy as np
import pytest


def word(r, g, b, a=0xFF):
    return (a << 24) | (b << 16) | (g << 8) | r


def test_all_equal_block(ort):
    for s in (2, 4, 8):
        f = np.full((s, s), 0xFF102030, np.uint32)
        assert ort.box_downsample(f, s).tolist() == [[0xFF102030]]


def test_half_rounds_up(ort):
    # R: 1 + 2 + 2 + 1 = 6, mean 1.5 -> 2
    f = np.array([[0xFF000001, 0xFF000002], [0xFF000002, 0xFF000001]], np.uint32)
    assert ort.box_downsample(f, 2).tolist() == [[0xFF000002]]
    # R: 0 + 0 + 0 + 1 = 1, mean 0.25 -> 0;  0 + 1 + 1 + 1 = 3, mean 0.75 -> 1
    f = np.array([[0xFF000000, 0xFF000000, 0xFF000000, 0xFF000001],
                  [0xFF000000, 0xFF000001, 0xFF000001, 0xFF000001]], np.uint32)
    assert ort.box_downsample(f, 2).tolist() == [[0xFF000000, 0xFF000001]]


def test_channels_do_not_carry(ort):
    # R: 255 + 255 + 255 + 254 = 1019 -> (1019 + 2) >> 2 = 255
    # G: 0 + 0 + 0 + 1 = 1 -> 0 (a carry out of R's sum would show here)
    # B: 255 + 0 + 255 + 0 = 510 -> 128;  A: 255
    f = np.array([[0xFFFF00FF, 0xFF0000FF], [0xFFFF00FF, 0xFF0001FE]], np.uint32)
    assert ort.box_downsample(f, 2).tolist() == [[0xFF8000FF]]


def test_s4_block(ort):
    # R: 15 x 10 + 18 = 168 -> (168 + 8) >> 4 = 11 (mean 10.5);  G: 8 x 255 -> (2040 + 8) >> 4 = 128
    # B: 16 x 255 -> 255;  A: 255
    f = np.empty(16, np.uint32)
    for k in range(16):
        f[k] = word(18 if k == 5 else 10, 255 if k % 2 else 0, 255)
    assert ort.box_downsample(f.reshape(4, 4), 4).tolist() == [[word(11, 128, 255)]]


def test_s8_block(ort):
    # R: 32 x 1 -> (32 + 32) >> 6 = 1 (mean 0.5);  G: 63 x 255 + 254 = 16319 -> (16319 + 32) >> 6 = 255
    # B: 64 x 200 -> 200;  A: 255
    f = np.empty(64, np.uint32)
    for k in range(64):
        f[k] = word(k & 1, 254 if k == 63 else 255, 200)
    assert ort.box_downsample(f.reshape(8, 8), 8).tolist() == [[word(1, 255, 200)]]


def test_frame_of_several_blocks(ort):
    # 4 x 6 samples, s = 2: 2 x 3 blocks, each with its own sums
    f = np.array([
        [word(0, 0, 0), word(4, 0, 0), word(1, 1, 1), word(1, 1, 1), word(255, 0, 9), word(255, 0, 9)],
        [word(0, 0, 0), word(4, 0, 0), word(1, 1, 1), word(2, 2, 2), word(255, 0, 9), word(255, 0, 10)],
        [word(7, 7, 7), word(7, 7, 7), word(0, 255, 0), word(0, 0, 255), word(3, 2, 1), word(3, 2, 1)],
        [word(7, 7, 7), word(7, 7, 7), word(255, 0, 0), word(0, 0, 0), word(3, 2, 1), word(4, 3, 2)],
    ], np.uint32)
    want = [[word(2, 0, 0), word(1, 1, 1), word(255, 0, 9)],         # 5/4 -> 1;  37/4 = 9.25 -> 9
            [word(7, 7, 7), word(64, 64, 64), word(3, 2, 1)]]        # 255/4 = 63.75 -> 64;  13/4 = 3.25 -> 3
    assert ort.box_downsample(f, 2).tolist() == want
    # leading axes (views) pass through
    assert ort.box_downsample(np.stack([f, f]), 2).tolist() == [want, want]


@pytest.mark.parametrize("s", [2, 4, 8])
def test_against_second_computation(ort, s):
    rng = np.random.default_rng(20 + s)
    f = rng.integers(0, 1 << 32, (3 * 8, 5 * 8), dtype=np.uint64).astype(np.uint32)
    h, w = f.shape[0] // s, f.shape[1] // s
    want = np.zeros((h, w), np.uint32)
    for c in range(4):
        ch = ((f >> (8 * c)) & 0xFF).astype(np.uint32).reshape(h, s, w, s)
        want |= ((ch.sum(axis=(1, 3)) + s * s // 2) >> (2 * int(np.log2(s)))).astype(np.uint32) << (8 * c)
    assert np.array_equal(ort.box_downsample(f, s), want)


def test_refuses_bad_arguments(ort):
    f = np.zeros((8, 8), np.uint32)
    with pytest.raises(ValueError):
        ort.box_downsample(f, 3)
    with pytest.raises(ValueError):
        ort.box_downsample(np.zeros((8, 6), np.uint32), 4)
