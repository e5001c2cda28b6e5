"""The compact 8-byte spring records (include/walker_hip.h wg_edge8; layout.pack_edges8): pack / unpack round trip,
eligibility by the (k, c) classes' float32 bit patterns, and invalidation when the spring records are edited."""
import numpy as np
import pytest

from walker_gym_amd.layout import compact_bytes_per_walker_step, layout_bytes_per_walker_step, pack, set_springs, \
    unpack_edges8
from walker_gym_amd.synthetic import canonical_walkers

# (M, K, A): 16, 4 and 1 walkers per 64-lane tile
SHAPES = [(4, 5, 2), (16, 40, 8), (64, 120, 8)]


def _spec(M, K, A, n_tiles_plus=1, seed=3):
    wpw = 64 // M
    N = 2 * wpw + n_tiles_plus          # two full tiles and a part of a third
    spec = canonical_walkers(N, seed=seed, M=M, K=K, A=A)
    spec["flags"] = (np.arange(N * K) % 7 == 3).astype(np.uint8)   # some strings, muscles among them
    return spec, N, wpw


@pytest.mark.parametrize("M,K,A", SHAPES)
def test_pack_unpack_round_trip(M, K, A):
    spec, N, wpw = _spec(M, K, A)
    lay = pack(spec)
    assert lay.edges8 is not None and lay.edges8.shape == (N * K, 2) and lay.edges8.dtype == np.uint32
    u = unpack_edges8(lay.edges8, M, K, A)
    e = np.arange(N * K)
    w, k = e // K, e % K
    assert np.array_equal(u["ei"], spec["ei"]) and np.array_equal(u["ej"], spec["ej"])
    assert np.array_equal(u["rest"].view(np.uint32), np.asarray(spec["rest"], np.float32).view(np.uint32))
    assert np.array_equal(u["muscle"], k < A)
    assert np.array_equal(u["string"], spec["flags"].astype(bool))
    # tile-relative byte addresses: the walker's place in its tile of 64 / M walkers
    assert np.array_equal(u["wt"], w % wpw)
    assert np.array_equal(u["bi"], ((w % wpw) * M + spec["ei"]) * 4)
    assert np.array_equal(u["bj"], ((w % wpw) * M + spec["ej"]) * 4)
    assert np.array_equal(u["xoff"], np.where(k < A, ((w % wpw) * A + k) * 4, 0))
    assert u["bi"].max() < 256 and u["bj"].max() < 256 and u["xoff"].max() < 256
    # the last walker of a full tile sits in the tile's last M lanes
    last = (w == wpw - 1)
    assert np.all(u["bi"][last] >> 2 >= 64 - M) and np.all(u["bj"][last] >> 2 >= 64 - M)
    # bits 24-29 are zero
    assert not np.any(lay.edges8[:, 0] & np.uint32(0x3f000000))
    assert np.array_equal(lay.kc, np.array([1000, 20, 1000, 20], np.float32))


def test_not_packed_for_other_shapes():
    assert pack(canonical_walkers(4, seed=1, M=25, K=60, A=10)).edges8 is None     # M does not divide 64
    from walker_gym_amd.synthetic import ragged_walkers
    assert pack(ragged_walkers(6, seed=1)).edges8 is None


def test_eligibility_by_class():
    M, K, A = 16, 40, 8
    spec = canonical_walkers(5, seed=2)
    mus = (np.arange(5 * K) % K) < A
    assert np.array_equal(pack(spec).kc, np.array([1000, 20, 1000, 20], np.float32))        # one class
    two = dict(spec, k=np.where(mus, 1000.0, 50.0).astype(np.float32), c=np.where(mus, 20.0, 5.0).astype(np.float32))
    lay = pack(two)
    assert lay.edges8 is not None and np.array_equal(lay.kc, np.array([1000, 20, 50, 5], np.float32))
    k3 = two["k"].copy()
    k3[K + A + 1] = 75.0                                                                    # a third k, one skeleton spring
    lay = pack(dict(two, k=k3))
    assert lay.edges8 is None and lay.kc is None
    k3 = two["k"].copy()
    k3[2 * K] = 999.0                                                                       # one muscle apart
    assert pack(dict(two, k=k3)).edges8 is None
    # bit patterns, not values: -0.0 damping against +0.0
    c0 = np.zeros(5 * K, np.float32)
    assert pack(dict(spec, c=c0)).edges8 is not None
    cm = c0.copy()
    cm[K + A + 3] = -0.0
    assert cm[K + A + 3] == 0.0 and pack(dict(spec, c=cm)).edges8 is None
    # no muscles: the muscle class takes the other class's pair
    lay = pack(canonical_walkers(5, seed=2, A=0))
    assert lay.edges8 is not None and not unpack_edges8(lay.edges8, M, K, 0)["muscle"].any()
    assert np.array_equal(lay.kc, np.array([1000, 20, 1000, 20], np.float32))


def test_set_springs_rebuilds_or_drops():
    M, K, A = 16, 40, 8
    spec = canonical_walkers(5, seed=4)
    lay = pack(spec)
    E = 5 * K
    mus = (np.arange(E) % K) < A
    # k of one class: still eligible, kc follows
    assert set_springs(lay, k=np.where(mus, 1000.0, 50.0)) is False
    assert lay.edges8 is not None and np.array_equal(lay.kc, np.array([1000, 20, 50, 20], np.float32))
    assert np.array_equal(lay.edges[:, 2].view(np.float32), np.where(mus, 1000.0, 50.0).astype(np.float32))
    # topology: endpoints swapped on one spring -> records and incidence lists follow
    ei, ej = np.asarray(spec["ei"]).copy(), np.asarray(spec["ej"]).copy()
    ei[K + 20], ej[K + 20] = 3, 9
    inc_before = lay.inc.copy()
    assert set_springs(lay, ei=ei, ej=ej) is True
    u = unpack_edges8(lay.edges8, M, K, A)
    assert np.array_equal(u["ei"], ei) and np.array_equal(u["ej"], ej)
    ref = pack(dict(spec, ei=ei, ej=ej, k=np.where(mus, 1000.0, 50.0).astype(np.float32)))
    assert np.array_equal(lay.edges, ref.edges) and np.array_equal(lay.edges8, ref.edges8)
    assert np.array_equal(lay.inc, ref.inc) and np.array_equal(lay.inc_off, ref.inc_off)
    assert not np.array_equal(lay.inc, inc_before)
    # string flags and rest lengths
    fl = np.zeros(E, np.uint8)
    fl[K + 30] = 1
    set_springs(lay, flags=fl, rest=np.asarray(spec["rest"]) * np.float32(1.5))
    u = unpack_edges8(lay.edges8, M, K, A)
    assert np.array_equal(u["string"], fl.astype(bool))
    assert np.array_equal(u["rest"], (np.asarray(spec["rest"]) * np.float32(1.5)).astype(np.float32))
    # a third k: dropped; back to two classes: rebuilt
    k3 = np.where(mus, 1000.0, 50.0)
    k3[K + 12] = 75.0
    set_springs(lay, k=k3)
    assert lay.edges8 is None and lay.kc is None
    set_springs(lay, k=1000.0)
    assert lay.edges8 is not None and np.array_equal(lay.kc, np.array([1000, 20, 1000, 20], np.float32))


def test_compact_bytes():
    full = layout_bytes_per_walker_step(16, 40, 8, 152)
    assert full == 2634                                   # the figure bench.py prints stays what it was
    assert compact_bytes_per_walker_step(16, 40, 8, 152, last=True) == full - 320
    assert compact_bytes_per_walker_step(16, 40, 8, 152) == full - 320 - 208
