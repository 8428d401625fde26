"""CPU (-m "not gpu"): dmvs_zpad_live_mask -- the one statement of which (plane, depth tap) pairs of a 3x3x3 layer meet a plane
that is not zero padding, from which every kernel behind dmvs_tune("zpad_skip") derives what it leaves out -- against a brute-force
enumeration that never evaluates the library's expression: each form is run on an indicator volume (1 inside, 0 in the padding)
through its textbook definition, and a pair is live when it picks up a 1."""
import numpy as np
import pytest

from dmvsnet_amd import _lib

S1, S2, T2 = 0, 1, 2


def _brute(form, D, oz0, TZ):
    """bit 3 * p + kz for plane oz0 + p of the tile."""
    pad = np.zeros(D + 4, dtype=np.int64)   # indicator of the input volume, index z + 2
    pad[2:D + 2] = 1
    mask = 0
    if form in (S1, S2):
        s = 1 if form == S1 else 2
        Do = (D + 2 - 3) // s + 1           # output planes of a k3 / pad 1 / stride s convolution
        for p in range(TZ):
            oz = oz0 + p
            if oz >= Do:
                continue
            for kz in range(3):
                mask |= int(pad[s * oz - 1 + kz + 2]) << (3 * p + kz)
        return mask
    # transposed k3 s2 p1 output_padding 1 (D -> 2 D), SCATTER definition: input plane j reaches output plane 2 j - 1 + kz.
    # The kernels gather on the input grid: base plane z owns output planes 2 z (tap 1) and 2 z + 1 (taps 2 and 0).
    reach = {}                               # (output plane, kz) -> an input plane inside the volume feeds it
    for j in range(-1, D + 2):
        for kz in range(3):
            reach[(2 * j - 1 + kz, kz)] = bool(pad[j + 2])
    for p in range(TZ):
        z = oz0 + p
        if z >= D:
            continue
        for kz in range(3):
            out_plane = 2 * z + (0 if kz == 1 else 1)
            mask |= int(reach[(out_plane, kz)]) << (3 * p + kz)
    return mask


@pytest.mark.parametrize("form", [S1, S2, T2])
def test_live_mask_matches_the_enumeration(form):
    lib = _lib.load()
    for D in range(1, 10):
        for TZ in (1, 2, 3, 4):
            for oz0 in range(0, D + 3):      # every tile origin, tiles that reach or lie past the last plane included
                assert lib.dmvs_zpad_live_mask(form, D, oz0, TZ) == _brute(form, D, oz0, TZ), (form, D, oz0, TZ)


def test_dead_shares_of_whole_volumes():
    """The shares the skipping kernels are sized by: 2 of 3 D (stride 1), 1 of 3 D / 2 (stride 2, even D), 1 of 3 D (transposed)."""
    lib = _lib.load()
    for D in (2, 4, 8):
        live = lambda form, planes: sum(bin(lib.dmvs_zpad_live_mask(form, D, z, 1)).count("1") for z in range(planes))  # noqa: E731
        assert live(S1, D) == 3 * D - 2
        assert live(S2, D // 2) == 3 * (D // 2) - 1
        assert live(T2, D) == 3 * D - 1
    assert lib.dmvs_zpad_live_mask(S1, 1, 0, 1) == 0b010          # depth 1: the middle tap only (what the @d1 forms compute)
    assert lib.dmvs_zpad_live_mask(S2, 5, 2, 1) == 0b011          # odd depth: the last output plane's tap 2 reads plane D
    assert lib.dmvs_zpad_live_mask(T2, 3, 2, 2) == 0b000110       # last input plane: tap 0 reads plane D; the plane after it: nothing


def test_bad_arguments():
    lib = _lib.load()
    for args in ((-1, 4, 0, 2), (3, 4, 0, 2), (S1, 0, 0, 2), (S1, 4, -1, 2), (S1, 4, 0, 0), (S1, 4, 0, 11)):
        assert lib.dmvs_zpad_live_mask(*args) == -1, args
    assert lib.dmvs_zpad_live_mask(S1, 4, 0, 10) >= 0


def test_zpad_skip_knob_arguments():
    lib = _lib.load()
    try:
        assert lib.dmvs_tune(b"zpad_skip", 0) == 0
        assert lib.dmvs_tune(b"zpad_skip", 1) == 0
        for bad in (-1, 2, 8):
            assert lib.dmvs_tune(b"zpad_skip", bad) == _lib.EINVAL
        assert lib.dmvs_tune(b"zpad_skipp", 1) == _lib.EUNSUPPORTED
    finally:
        assert lib.dmvs_tune(b"zpad_skip", 1) == 0
