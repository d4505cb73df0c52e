"""CPU: the table of tests/_index_layouts.py reaches what it names -- REQUIRED here by assertion, on the numpy restatement of the grid
geometry (tests/_radius.grid_dims) and on the brute forces themselves, so that tests/test_kd_index_layouts_gpu.py cannot pass
without the device having walked a 1024 x 1 x 1 grid with most points clamped, a 2 x 2 x 2 grid of 6.8e-31 m cells, ragged tiles, a
single tile of more than 4096 records and a handle built twice; and the answers it compares are neither all hits nor all misses."""
import numpy as np
import pytest

from tests import _index_layouts as IL
from tests import _radius as R
from tests import _segment as G

LEG = IL.LEG
FINITE = (0.0625, 4.0)
REFS = ("line", "thick_line", "plane0", "plane", "diag", "same", "two", "tiles", "swept", "rebuilt", "ties")


def test_the_table_is_complete_and_within_its_size():
    lays = IL.layouts()
    assert tuple(lays) == IL.NAMES and {l.ref for l in lays.values()} == set(REFS)
    for lay in lays.values():
        assert max(len(c) for c in lay.clouds) <= 12289 and lay.cap <= 12289
        assert lay.path.shape == (len(lay.clouds), IL.N_POINTS, 3) and lay.path.dtype == np.float64 and np.isfinite(lay.path).all()
        same = [o for o in lays.values() if o.ref == lay.ref]
        assert all(o.clouds is lay.clouds or all(np.array_equal(a, b, equal_nan=True) for a, b in zip(o.clouds, lay.clouds)) for o in same)
        assert all(np.array_equal(o.path, lay.path) for o in same)
        for s, c in enumerate(lay.clouds):
            if len(R.kept(c)):
                p = lay.path[s]
                assert (p[10] == p[11]).all() and (R.kept(c).astype(np.float64) == p[10]).all(axis=1).any()      # a degenerate leg ON a stored point
                assert abs(np.linalg.norm(p[12] - p[11]) - 0.01) < 1e-12 and abs(np.linalg.norm(p[9] - p[8]) - 1e6) < 1e-6
                far = np.sqrt(min(G.seg_dists(R.kept(c), p[7], p[8])[0].min(), 1e300))
                assert 90.0 < far < 200.0, (lay.name, s, far)


@pytest.mark.parametrize("name", IL.DEGENERATE)
def test_degenerate_grids_have_the_intended_shape(name):
    lay = IL.layouts()[name]
    g, nt = R.grid_dims(lay.clouds[0])
    assert tuple(int(x) for x in g) == lay.shape and nt == (len(lay.clouds[0]) + IL.TILE - 1) // IL.TILE
    if name in ("same", "two"):
        h = IL.grid_of(lay.clouds[0])[2]
        assert (6.8e-31 < h < 6.9e-31) if name == "same" else (0.68 < h < 0.69)


@pytest.mark.parametrize("name", ["line", "thick_line"])
def test_most_of_a_line_is_clamped_into_the_last_cell(name):
    lay = IL.layouts()[name]
    c, p = lay.clouds[0], lay.path[0]
    cells, g = IL.true_cells(c)
    assert tuple(g) == (1024, 1, 1)
    beyond = cells[:, 0] > g[0] - 1
    assert beyond.mean() >= 0.80, beyond.mean()
    if name == "line":
        assert beyond.sum() == 982
    _, lo, h = IL.grid_of(c)
    covered = lo[0] + 1024 * h
    # the cast along the cloud takes 1024 slabs, both ways; a leg inside the clamped part spans no cell; one leg leaves the clamped part
    slabs = [IL.cast_slabs(c, p[j], p[j + 1]) for j in range(12)]
    assert slabs[LEG["along"]] == 1024 and slabs[LEG["back"]] == 1024 and slabs[LEG["inner"]] == 1
    a, b = p[LEG["inner"]], p[LEG["inner"] + 1]
    assert min(a[0], b[0]) > covered and a[1] == b[1] and a[2] == b[2]
    if name == "line":
        assert {a[0], b[0]} == {50.0, 60.0} and a[1] == 0 and a[2] == 0
        assert (G.seg_dists(c, a, b)[0] == 0).sum() == 81 and (G.seg_dists(c, p[0], p[1])[0] == 0).sum() > 512      # IN the line: only t differs
    a, b = p[LEG["into_grid"]], p[LEG["into_grid"] + 1]
    assert a[0] > covered > b[0] > lo[0] and slabs[LEG["into_grid"]] > 100


def test_planes_have_one_layer_of_cells_and_a_leg_with_two_equal_nearest_points():
    for name in ("plane0", "plane"):
        lay = IL.layouts()[name]
        c, p = lay.clouds[0], lay.path[0]
        assert (c[:, 2] == 0).all() == (name == "plane0") and np.abs(c[:, 2]).max() < 0.01
        a, b = p[LEG["across"]], p[LEG["across"] + 1]
        assert a[0] == b[0] and a[1] == b[1] and a[2] < c[:, 2].min() and b[2] > c[:, 2].max()
        d = np.sort(G.seg_dists(c, a, b)[0])
        assert d[0] == d[1] < d[2]
        a, b = p[LEG["inner"]], p[LEG["inner"] + 1]
        assert a[2] == b[2] and c[:, 2].min() <= a[2] <= c[:, 2].max()                                          # a leg IN the plane


def test_the_ragged_handle_holds_zero_to_four_tiles():
    clouds = IL.tile_clouds()
    assert [len(c) for c in clouds] == list(IL.TILE_SIZES)
    per_tile = [IL.tiles_kept(c) for c in clouds]
    assert [len(t) for t in per_tile] == [1, 1, 2, 2, 3, 1, 1, 1, 4, 0, 1]
    assert per_tile[8][2] == 0 and per_tile[8][3] == 1                       # a tile that is all NaN-x, and one point behind it
    assert per_tile[2][1] == 1 and per_tile[4][2] == 1                       # one point in the last tile
    for s in (3, 4, 8):
        assert np.isnan(clouds[s][4090:4110, 0]).all()                       # the NaN-x run across the first tile boundary
    for s, c in enumerate(clouds):
        assert int(np.isnan(c[:, 0]).sum()) >= (37 if len(c) > 600 else 0) and sum(per_tile[s]) == len(R.kept(c))
    for stride in (3, 4):
        lay = IL.layouts()[f"tiles_s{stride}"]
        assert lay.stride == stride and lay.cap == 12289 and (lay.cap + IL.TILE - 1) // IL.TILE == 4


def test_the_swept_keyframe_holds_more_than_a_tile_in_one_tile():
    sw = IL.swept()
    assert [len(c) for c in sw["keyframe"]] == [8193, 4200, 300] and [len(c) for c in sw["current"]] == [600, 600, 1]
    assert sw["current"][0][:, 0].max() < 3.0 and sw["current"][1][:, 0].max() > 25.0
    sizes = [len(a) for a in sw["after"]]
    assert sw["rebuilt"] == [1, 1, 0] and sw["outliers"][:2] == sizes[:2] and sw["outliers"][2] == 0
    assert IL.TILE < sizes[0] < 8193 and 0 < sizes[1] < 4200 and sizes[2] == 300, sizes
    assert sw["after"][2] is not None and np.array_equal(sw["after"][2], sw["keyframe"][2])                      # left untouched
    # the survivors are a subsequence of the keyframe, order preserved, and every one is farther than th from the current frame
    kf, after = sw["keyframe"][0], sw["after"][0]
    pos = np.flatnonzero((kf[:, None, 0] == after[None, :200, 0]).any(axis=1))[:5]
    assert len(pos) == 5 and (np.diff(pos) > 0).all()
    for q in after[::500].astype(np.float64):
        assert np.sqrt(R.sq_dists(sw["current"][0], q).min()) > IL.SWEEP_TH
    lay = IL.layouts()["swept"]
    assert lay.how == "sweep" and lay.cap == 8193 and [len(c) for c in lay.clouds] == sizes


def test_the_second_build_is_smaller_and_elsewhere():
    first, second = IL.rebuilt()
    assert [len(c) for c in first] == [8193, 4097, 600, 5000] and [len(c) for c in second] == [513, 0, 1, 4097]
    assert (len(first[0]) + IL.TILE - 1) // IL.TILE == 3 and (len(second[0]) + IL.TILE - 1) // IL.TILE == 1      # two stale tiles
    assert len(second[3]) > len(first[2]) and first[0][:, 0].max() > 25.0 and second[0][:, 0].min() < -3.0
    a, b = IL.layouts()["rebuilt"], IL.layouts()["rebuilt_fresh"]
    assert a.how == "rebuild" and b.how == "build" and a.ref == b.ref and a.cap == b.cap == 8193


def test_the_quantised_clouds_tie():
    lays = IL.layouts()
    assert [lays[n].ties for n in ("ties_default", "ties_nanoflann", "ties_auto")] == [0, 1, 2]
    lay = lays["ties_default"]
    assert [len(c) for c in lay.clouds] == [6000, 4097]
    for s, c in enumerate(lay.clouds):
        k = R.kept(c)
        assert (k / IL.QUANTUM == np.round(k / IL.QUANTUM)).all()
        for j in (LEG["along"], LEG["across"], LEG["on_point"]):
            d = np.sort(G.seg_dists(k, lay.path[s, j], lay.path[s, j + 1])[0])
            assert any(d[kk - 1] == d[kk] for kk in IL.NEAREST_K), (s, j)


@pytest.mark.parametrize("ref", REFS)
def test_every_answer_set_has_hits_and_misses(ref):
    S = IL.want_cast(ref, 0.0)["hit"].shape[0]
    nonempty = [s for s in range(S) if len(R.kept(IL._by_ref(ref).clouds[s]))]
    rc = np.stack([IL.want_radius(ref, r2, 0)["counts"][nonempty] for r2 in FINITE])
    sc = np.stack([IL.want_segment(ref, r2, 0)["counts"][nonempty] for r2 in FINITE])
    hit = np.stack([IL.want_cast(ref, r2)["hit"][nonempty] for r2 in FINITE])
    t = np.stack([IL.want_cast(ref, r2)["t"][nonempty] for r2 in FINITE])
    for what, a in (("radius", rc), ("segment", sc), ("cast", hit)):
        assert (a > 0).any() and (a == 0).any(), (ref, what)
    assert ((t > 0) & (t < 1)).any() and ((t == 0) & (hit == 1)).any(), ref      # a first contact on the way, and inside at the start
    if ref not in ("same", "two"):
        assert rc.max() > 64 or sc.max() > 64                                     # a list that k = 64 cuts
    # radius 0 gives nothing (the tests are strict), an infinite one everything
    usable = np.array([int(np.isfinite(R.kept(c)).all(axis=1).sum()) for c in IL._by_ref(ref).clouds])
    assert (IL.want_radius(ref, 0.0, 0)["counts"] == 0).all() and (IL.want_segment(ref, IL.INF, 0)["counts"] == usable[:, None]).all()
    for k in IL.NEAREST_K:
        assert (IL.want_nearest(ref, k)["counts"] == np.minimum(k, usable)[:, None]).all()
    stops = np.concatenate([IL.want_path_cast(ref, r2, w)["stop"][nonempty] for r2 in IL.RADII for w in IL.WINDOWS])
    legs = np.concatenate([IL.want_path_cast(ref, r2, w)["leg"][nonempty] for r2 in FINITE for w in IL.WINDOWS])
    assert set(stops.tolist()) == {0, 1} and len(set(legs.tolist())) >= 2, (ref, set(legs.tolist()))


@pytest.mark.parametrize("name", ["line", "plane0"])
def test_a_list_is_cut_inside_a_run_of_equal_distances(name):
    lay = IL.layouts()[name]
    cut = set()
    for j in range(12):
        d = np.sort(G.seg_dists(lay.clouds[0], lay.path[0, j], lay.path[0, j + 1])[0])
        cut |= {k for k in IL.NEAREST_K if d[k - 1] == d[k]}
    assert cut == (set(IL.NEAREST_K) if name == "line" else {1}), cut


@pytest.mark.parametrize("name", ["same", "two"])
def test_coincident_points_are_met_on_the_way_and_at_the_start(name):
    """with cells of 6.8e-31 m (`same`) every coordinate difference times 1 / h is astronomically large before the clamp"""
    lay = IL.layouts()[name]
    p = lay.path[0]
    _, lo, h = IL.grid_of(lay.clouds[0])
    if name == "same":
        assert (np.abs(p[0] - lo).max() / h) > 1e30
    on_the_way, at_start = IL.want_cast(name, 0.0625), IL.want_cast(name, 4.0)
    j = LEG["along"]
    assert on_the_way["hit"][0, j] == 1 and 0 < on_the_way["t"][0, j] < 1 and at_start["hit"][0, j] == 1 and at_start["t"][0, j] == 0
    assert on_the_way["indices"][0, j] == 0                                        # coincident points: the lowest index
    if name == "two":
        assert set(at_start["indices"][0][at_start["hit"][0] == 1].tolist()) >= {0, 100} or on_the_way["indices"][0, LEG["back"]] == 100


@pytest.mark.parametrize("ref", REFS)
def test_hit_is_count_above_zero_away_from_the_radius(ref):
    """the identity the GPU test applies to the device's answers holds on the references, inside the 95 % cap"""
    lay = IL._by_ref(ref)
    for r2 in FINITE:
        clear = IL.clear_legs(lay, r2)
        assert clear.mean() >= 0.95, (ref, r2, clear.mean())
        hit, cnt = IL.want_cast(ref, r2)["hit"], IL.want_segment(ref, r2, 0)["counts"]
        assert np.array_equal(hit[clear] > 0, cnt[clear] > 0), (ref, r2)


def test_the_frame_list_mixes_three_builders_and_several_frames_answer():
    fl = IL.frame_list()
    assert [[len(c) for c in h] for h in fl["held"]] == [[6000, len(IL.swept()["after"][s]), n] for s, n in enumerate((513, 0, 4097))]
    assert [len(c) for c in fl["first"]] == [8193, 4097, 5000] and fl["path"].shape == (3, 13, 3)
    for r2 in FINITE:
        f = IL.want_frames("cast", r2)["frame"]
        assert {0, 1} <= set(f.reshape(-1).tolist()), (r2, f)
        sf = IL.want_frames("segment", r2, 64)["frame"]
        assert {0, 1, 2} <= set(sf[[0, 2]].reshape(-1).tolist()) and 2 not in sf[1]                              # scene 1's third frame is empty
    nf = IL.want_frames("nearest", 64)["frame"]
    assert all(len(set(nf[s, j].tolist())) >= 2 for s in (0, 2) for j in (LEG["along"], LEG["across"]))
    stops = np.concatenate([IL.want_frames("path_cast", r2, w)["stop"] for r2 in IL.RADII for w in IL.WINDOWS])
    frames = np.concatenate([IL.want_frames("path_cast", r2, w)["frame"] for r2 in FINITE for w in IL.WINDOWS])
    assert set(stops.tolist()) == {0, 1} and len(set(frames.tolist()) - {-1}) >= 2
    assert (IL.want_frames("radius", 4.0, 0)["counts"] > 64).any() and (IL.want_frames("radius", 0.0625, 0)["counts"] == 0).any()
