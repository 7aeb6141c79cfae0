"""turtle_amd_tally_n (k_tally) against sharding.tally_reference, exactly: every size at which the
kernel changes its path -- less than a wave, a wave and one ray more, more than one block, more than
one trip of a block -- few media (counted by ballots) and all rays in one (the contended word), every
histogram from one bin to the largest that fits in LDS (one shared copy; the small ones have a copy
a wave), that size plus one (refused), media outside [-1, n_media), and the lengths at the edges of
the histogram.  In both spaces, and accumulating over two calls."""
import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import sharding

pytestmark = pytest.mark.gpu

LENGTH_MAX = 1000.0
SIZES = (1, 63, 64, 65, 257, 4099, 100_003)
MEDIA = (1, 2, 5)
EDGES = (np.nan, -1.0, 0.0, LENGTH_MAX, np.nextafter(LENGTH_MAX, 0.0), np.inf)


def largest_bins(n_media):
    """(n_media + 1 + n_bins + 1) 32-bit counters within 64 KB of LDS"""
    return 64 * 1024 // 4 - 2 - n_media


def bins_of(n_media):
    return (1, 7, 1024, largest_bins(n_media))


def rays(n, n_media, seed, one_medium=None):
    rng = np.random.default_rng(seed)
    index = np.empty((n, 2), dtype=np.int32)
    # media -2 and n_media (counted nowhere) and -1 (no medium: hits[0]) among the real ones
    index[:, 0] = rng.integers(-2, n_media + 1, n) if one_medium is None else one_medium
    index[:, 1] = rng.integers(-1, 3, n)
    length = rng.uniform(0.0, 1.05 * LENGTH_MAX, n)
    at = rng.permutation(n)[: len(EDGES)]
    length[at] = EDGES[: len(at)]
    return index, length


def reference(index, length, n_media, n_bins):
    """tally_reference; its bincount takes no medium below -1, which the library counts nowhere, so
    it is given the hits' rows without those and the histogram's rows whole"""
    keep = index[:, 0] >= -1
    hits, _ = sharding.tally_reference(index[keep], length[keep], n_media, n_bins, LENGTH_MAX)
    _, histogram = sharding.tally_reference(np.zeros_like(index), length, n_media, n_bins, LENGTH_MAX)
    return hits, histogram


def in_space(space, *arrays):
    if space == "host":
        return arrays
    import torch
    there = tuple(torch.as_tensor(a, device="cuda") for a in arrays)
    torch.cuda.synchronize()             # (the library launches on a stream of its own)
    return there


def tally(space, index, length, n_media, n_bins, into=None):
    """TA.tally into arrays of the test's own making: zeroed, and the zeroing done, before the
    library's stream adds to them"""
    if into is None:
        into = (np.zeros(n_media + 1, dtype=np.int64), np.zeros(n_bins + 1, dtype=np.int64))
    hits, histogram = in_space(space, *into) if isinstance(into[0], np.ndarray) else into
    return TA.tally(*in_space(space, index, length), n_media, n_bins, LENGTH_MAX, hits=hits, histogram=histogram)


def host(a):
    if isinstance(a, np.ndarray):
        return a
    TA.synchronize()
    return a.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    """the rays of every (n, n_media), drawn once"""
    return {(n, m): rays(n, m, seed=1000 * m + n % 997) for n in SIZES for m in MEDIA}


@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("n_media", MEDIA)
@pytest.mark.parametrize("n", SIZES)
def test_tally_equals_the_reference(cases, n, n_media, space):
    index, length = cases[(n, n_media)]
    for n_bins in bins_of(n_media):
        ref_hits, ref_histogram = reference(index, length, n_media, n_bins)
        assert ref_histogram.sum() == n
        hits, histogram = tally(space, index, length, n_media, n_bins)
        assert np.array_equal(host(hits), ref_hits), n_bins
        assert np.array_equal(host(histogram), ref_histogram), n_bins
        # a second call adds to the first's arrays
        tally(space, index, length, n_media, n_bins, into=(hits, histogram))
        assert np.array_equal(host(hits), 2 * ref_hits), n_bins
        assert np.array_equal(host(histogram), 2 * ref_histogram), n_bins


@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("n_media", MEDIA)
def test_all_rays_in_one_medium(n_media, space):
    """every lane of every wave adds to the same word of the hits, and to one bin"""
    n = SIZES[-1]
    for medium in (-1, n_media - 1):
        index, length = rays(n, n_media, seed=7, one_medium=medium)
        length[:] = 0.5 * LENGTH_MAX
        hits, histogram = tally(space, index, length, n_media, 7)
        ref_hits, ref_histogram = reference(index, length, n_media, 7)
        assert ref_hits[medium + 1] == n and ref_histogram[3] == n
        assert np.array_equal(host(hits), ref_hits) and np.array_equal(host(histogram), ref_histogram)


def test_more_media_than_the_ballots_take():
    """beyond a few media the hits are counted in LDS, as the histogram"""
    n, n_media = 4099, 40
    index, length = rays(n, n_media, seed=11)
    for n_bins in (7, largest_bins(n_media)):
        hits, histogram = tally("device", index, length, n_media, n_bins)
        ref_hits, ref_histogram = reference(index, length, n_media, n_bins)
        assert np.array_equal(host(hits), ref_hits) and np.array_equal(host(histogram), ref_histogram)


@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("n_media", MEDIA)
def test_one_bin_too_many_is_refused(n_media, space):
    index, length = rays(65, n_media, seed=3)
    with pytest.raises(TA.TurtleError):
        tally(space, index, length, n_media, largest_bins(n_media) + 1)
