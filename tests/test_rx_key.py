"""api.RxKey on CPU tensors against a plain Python loop: key[c][b] = 1 iff channel c has no band (band -1) or its band was
present in one of the stream blocks b - hold .. b; blocks in front of the first call are off, the carry crosses calls, any
non-zero verdict byte counts, reset() forgets the carry, and a band the spectrum does not have is refused."""
import numpy as np
import pytest

from hackrfdiags_amd import api


def rxkey_loop(present, band, hold):
    n, C_ = present.shape[0], len(band)
    key = np.zeros((C_, n), dtype=np.uint8)
    for c in range(C_):
        for b in range(n):
            if band[c] < 0:
                key[c, b] = 1
            else:
                key[c, b] = int(any(present[j, band[c]] != 0 for j in range(max(0, b - hold), b + 1)))
    return key


BAND = [2, -1, 0, 5, 2, 4]                                     # channel 1 always on, channels 0 and 4 share a band
K, N = 6, 40


def stream(seed):
    rng = np.random.default_rng(seed)
    present = ((rng.integers(0, 7, size=(N, K)) == 0) * rng.integers(1, 256, size=(N, K))).astype(np.uint8)
    present[:, 4] = 0
    present[7, 4] = 0x80                                       # one block present: exactly hold + 1 keys
    return present


@pytest.mark.parametrize("hold", [0, 1, 3])
@pytest.mark.parametrize("cut", [1, 2, 5])
def test_rxkey_equals_a_plain_loop(hold, cut):
    import torch
    present = stream(10 * hold + cut)
    assert (present > 1).any(), "bytes other than 1"
    want = rxkey_loop(present, BAND, hold)
    assert want[5].sum() == hold + 1 and want[5, 7] == 1 and want[1].all() and (want[0] == want[4]).all()
    rk = api.RxKey(len(BAND), BAND, hold=hold)
    got = []
    for at in range(0, N, cut):
        part = torch.from_numpy(present[at:at + cut].copy())
        k = rk(part[0] if cut == 1 else part)                  # a [K] tensor counts as one block
        assert k.dtype == torch.uint8 and tuple(k.shape) == (len(BAND), cut) and k.is_contiguous()
        got.append(k.numpy())
    got = np.concatenate(got, axis=1)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert set(np.unique(got)) <= {0, 1}


def test_rxkey_reset_forgets_the_carry():
    import torch
    present = np.zeros((3, K), dtype=np.uint8)
    present[2, 0] = 3                                          # channel 2's band, in the call's last block
    rk = api.RxKey(len(BAND), BAND, hold=2)
    assert rk(torch.from_numpy(present)).numpy()[2].tolist() == [0, 0, 1]
    quiet = torch.zeros((3, K), dtype=torch.uint8)
    assert rk(quiet).numpy()[2].tolist() == [1, 1, 0], "held over the call's edge"
    rk(torch.from_numpy(present))
    rk.reset()
    k = rk(quiet).numpy()
    assert k[2].tolist() == [0, 0, 0] and k[1].tolist() == [1, 1, 1], "after reset only the band-less channel is on"


def test_rxkey_refuses():
    import torch
    with pytest.raises(ValueError):
        api.RxKey(2, [0, K])(torch.zeros((1, K), dtype=torch.uint8))       # band K of K bands
    with pytest.raises(ValueError):
        api.RxKey(2, [0, 1, 2])                                # one band per channel
    with pytest.raises(ValueError):
        api.RxKey(0, [])
    with pytest.raises(ValueError):
        api.RxKey(2, [0, 1], hold=-1)
    assert api.RxKey(2, [0, K - 1])(torch.zeros((1, K), dtype=torch.uint8)).shape == (2, 1)
