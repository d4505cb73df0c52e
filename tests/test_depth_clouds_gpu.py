"""GPU: amk_depth_to_clouds (AddVertex's image half, ProcessDepth followed by BuildEdgeCloud, for down-scaled images of any size)
against oracle/depth_oracle.c: identical float32 bits, counts and order of both clouds -- above the one-block kernels' 16 000 pixels,
at every band border of a small image (the internal hook amk__depth_set_band_rows tiles images of any size), on degenerate images;
the same bytes as amk_depth_to_cloud + amk_depth_to_edge_cloud where those run; the refusals; and depth frames above the old limit
through the pipeline."""
import ctypes as C

import numpy as np
import pytest

from tests import _oracle
from tests._depth import TBC, poses as _poses, wall_scene as _wall_scene
from tests.test_depth_oracle import YAML

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture
def band_rows():
    """Sets the band height of the tiled path (0: automatic dispatch) and puts the automatic one back afterwards."""
    from avoid_mpc_amd import capi
    lib = capi.load()
    try:
        yield lambda r: lib.amk__depth_set_band_rows(int(r))
    finally:
        lib.amk__depth_set_band_rows(0)


def _references(imgs, prm, Twb, Twc):
    """Per scene (obstacle cloud, edge cloud, edge map) of the oracle; an empty obstacle cloud empties the edge cloud (:126-128)."""
    refs = []
    for s in range(len(imgs)):
        cloud, _ = _oracle.depth_oracle(imgs[s], prm, Twb[s])
        edge, _, _, emap = _oracle.depth_edge_oracle(imgs[s], prm, Twc[s])
        refs.append((cloud, edge if len(cloud) else edge[:0], emap))
    return refs


def _run(torch, imgs, prm, Twb, Twc, stride=3):
    from avoid_mpc_amd.host import depth_params, depth_to_clouds
    dev = torch.from_numpy(imgs.view(np.int16) if imgs.dtype == np.uint16 else imgs).cuda()
    out = depth_to_clouds(dev, depth_params(**prm), torch.from_numpy(Twb).cuda(), torch.from_numpy(Twc).cuda(), point_stride=stride)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _assert_equal(got, refs, what=""):
    cloud, counts, edge, ecounts = got
    for s, (rc, re, _) in enumerate(refs):
        assert counts[s] == len(rc) and ecounts[s] == len(re), (what, s, counts[s], len(rc), ecounts[s], len(re))
        assert np.array_equal(cloud[s, :counts[s], :3].view(np.uint32), rc.view(np.uint32)), (what, s, "obstacle")
        assert np.array_equal(edge[s, :ecounts[s], :3].view(np.uint32), re.view(np.uint32)), (what, s, "edge")


_LARGE = {}


def _large_case(dtype):
    """240 x 320 at scale 1 (76 800 pixels), S = 4, and the oracle's answer, computed once per pixel type"""
    if dtype not in _LARGE:
        rng = np.random.default_rng(4)
        shape, S = (240, 320), 4
        imgs = np.stack([_wall_scene(rng, shape, dtype) for _ in range(S)])
        imgs[2] = 0
        imgs[3, :236] = 0
        prm = dict(YAML, pixel2meter=1e-3 if dtype == np.uint16 else 1.0, resize_scale=1.0, Tbc=TBC)
        Twb, Twc = _poses(rng, S), _poses(rng, S)
        _LARGE[dtype] = (imgs, prm, Twb, Twc, _references(imgs, prm, Twb, Twc))
    return _LARGE[dtype]


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_above_the_one_block_limit(dtype, stride, torch_cuda):
    """240 x 320 at scale 1: 76 800 pixels, the shape amk_depth_to_edge_cloud refuses; Twc != Twb; one scene all zero, one whose only
    valid pixels are in its last rows (whether a scene is empty is decided across bands)."""
    imgs, prm, Twb, Twc, refs = _large_case(dtype)
    got = _run(torch_cuda, imgs, prm, Twb, Twc, stride)
    print("counts", got[1], "edge counts", got[3], "oracle", [(len(a), len(b)) for a, b, _ in refs])
    _assert_equal(got, refs)
    assert got[1][2] == 0 and got[3][2] == 0
    assert min(got[3][s] for s in (0, 1, 3)) > 10 and min(got[1][s] for s in (0, 1, 3)) > 0


@pytest.mark.parametrize("shape", [(125, 128), (127, 126), (7, 2047)])
def test_at_the_edge_of_the_dispatch(shape, band_rows, torch_cuda):
    """Scale 1, float32, S = 2, the automatic band height: 125 x 128 = 16 000 pixels, the last size on the one-block pair (its LDS
    layers at their largest); 127 x 126 = 16 002, the first tiled size; 7 x 2047 = 14 329, an odd pixel count on one block (the
    magnitude layer starts at (npix + 1) & ~1) at the widest odd row.  3 x 5333 = 15 999 would be the odd count next to the limit,
    but its width is above AMK_DEPTH_MAX_WIDTH: the call refuses it (test_refusals)."""
    rng = np.random.default_rng(12)
    S = 2
    imgs = np.stack([_wall_scene(rng, shape, np.float32) for _ in range(S)])
    prm = dict(YAML, pixel2meter=1.0, resize_scale=1.0, Tbc=TBC)
    Twb, Twc = _poses(rng, S), _poses(rng, S)
    refs = _references(imgs, prm, Twb, Twc)
    assert all(len(rc) > 0 and len(re) > 10 for rc, re, _ in refs), [(len(rc), len(re)) for rc, re, _ in refs]
    band_rows(0)
    _assert_equal(_run(torch_cuda, imgs, prm, Twb, Twc), refs, shape)


BORDER_H, BORDER_W = 37, 53


@pytest.fixture(scope="module")
def border_case():
    """37 x 53 float32 at scale 1: a horizontal depth step (20 m above, 5 m from row r0 down) for every r0 in 1..36, a vertical step at
    column 20, a diagonal step -- and the oracle's answer, computed once."""
    H, W = BORDER_H, BORDER_W
    imgs = []
    for r0 in range(1, H):
        d = np.full((H, W), 20.0, np.float32)
        d[r0:] = 5.0
        imgs.append(d)
    d = np.full((H, W), 20.0, np.float32)
    d[:, 20:] = 5.0
    imgs.append(d)
    r, c = np.mgrid[0:H, 0:W]
    imgs.append(np.where(c > r + 8, np.float32(5.0), np.float32(20.0)).astype(np.float32))
    imgs = np.stack(imgs)
    rng = np.random.default_rng(9)
    prm = dict(YAML, resize_scale=1.0, Tbc=TBC, fx=30.0, fy=30.0, cx=26.0, cy=18.0)
    Twb, Twc = _poses(rng, len(imgs)), _poses(rng, len(imgs))
    return imgs, prm, Twb, Twc, _references(imgs, prm, Twb, Twc)


def test_band_border_precondition(border_case):
    """Every row holds an edge pixel of the oracle in at least one scene: every band boundary has edges on both sides, whatever the
    band height."""
    refs = border_case[4]
    rows_with_edges = np.zeros(BORDER_H, bool)
    for _, _, emap in refs:
        rows_with_edges |= emap.reshape(BORDER_H, BORDER_W).astype(bool).any(axis=1)
    assert rows_with_edges.all(), np.flatnonzero(~rows_with_edges)


@pytest.mark.parametrize("rows_per_band", [1, 2, 3, 5, 16, 37, 64])
def test_band_borders(rows_per_band, border_case, band_rows, torch_cuda):
    imgs, prm, Twb, Twc, refs = border_case
    band_rows(rows_per_band)
    _assert_equal(_run(torch_cuda, imgs, prm, Twb, Twc), refs, rows_per_band)


def _single_pixel_image():
    d = np.zeros((7, 65), np.float32)
    d[6, 30] = 5.0
    return d


@pytest.mark.parametrize("rows_per_band", [1, 0])
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 64), (7, 65), "single"])
def test_degenerate_images(shape, rows_per_band, band_rows, torch_cuda):
    """W = 1, H = 1, a width at a wavefront multiple and one past it; and a single valid pixel in the last row, around which the oracle
    finds more edge pixels than it keeps points (an eroded depth of 0 is below depth_min: the filter of FrameKDMap.cpp:201-203)."""
    rng = np.random.default_rng(3)
    if shape == "single":
        imgs = _single_pixel_image()[None]
    else:
        imgs = np.full((3,) + shape, 20.0) + rng.normal(0, 0.02, (3,) + shape)
        imgs[:, shape[0] // 2:, shape[1] // 2:] = 5.0                 # a near corner (the whole of a 1 x 1 image)
        imgs[1][rng.random(shape) < 0.1] = 0.0                        # invalid pixels
        imgs = imgs.astype(np.float32)
    prm = dict(YAML, resize_scale=1.0, Tbc=TBC, fx=30.0, fy=30.0, cx=2.0, cy=2.0)
    Twb, Twc = _poses(rng, len(imgs)), _poses(rng, len(imgs))
    refs = _references(imgs, prm, Twb, Twc)
    if shape == "single":
        assert len(refs[0][0]) == 1 and len(refs[0][1]) < int(refs[0][2].astype(bool).sum())
    band_rows(rows_per_band)
    _assert_equal(_run(torch_cuda, imgs, prm, Twb, Twc), refs, (shape, rows_per_band))


@pytest.mark.parametrize("rows_per_band", [0, 4])
@pytest.mark.parametrize("shape,scale", [((480, 640), 10.0), ((97, 131), 4.0)])
def test_same_bytes_as_the_two_calls(shape, scale, rows_per_band, band_rows, torch_cuda):
    torch = torch_cuda
    from avoid_mpc_amd.host import depth_params, depth_to_cloud
    rng = np.random.default_rng(6)
    S = 3
    imgs = np.stack([_wall_scene(rng, shape, np.uint16) for _ in range(S)])
    imgs[1] = 0
    prm = dict(YAML, pixel2meter=1e-3, resize_scale=scale, Tbc=TBC)
    Twb, Twc = _poses(rng, S), _poses(rng, S)
    dev = torch.from_numpy(imgs.view(np.int16)).cuda()
    cloud, counts = depth_to_cloud(dev, depth_params(**prm), torch.from_numpy(Twb).cuda())
    edge, ecounts = depth_to_cloud(dev, depth_params(**prm), torch.from_numpy(Twc).cuda(), edge=True)
    torch.cuda.synchronize()
    cloud, counts, edge, ecounts = (t.cpu().numpy() for t in (cloud, counts, edge, ecounts))
    band_rows(rows_per_band)
    got = _run(torch, imgs, prm, Twb, Twc)
    assert np.array_equal(got[1], counts) and np.array_equal(got[3], ecounts) and counts[0] > 0 and ecounts[0] > 10
    for s in range(S):
        assert np.array_equal(got[0][s, :counts[s]].view(np.uint32), cloud[s, :counts[s]].view(np.uint32))
        assert np.array_equal(got[2][s, :ecounts[s]].view(np.uint32), edge[s, :ecounts[s]].view(np.uint32))


def test_refusals(torch_cuda):
    torch = torch_cuda
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import depth_params
    lib = capi.load()
    rows, cols, S = 150, 200, 2                      # 30 000 pixels at scale 1: the tiled path
    p = depth_params(**dict(YAML, resize_scale=1.0))
    nbytes = C.c_longlong()
    assert lib.amk_depth_clouds_work_bytes(rows, cols, 1.0, S, C.byref(nbytes)) == capi.AMK_OK
    cap = rows * cols
    img = torch.full((S, rows, cols), 5.0, dtype=torch.float32, device="cuda")
    T = torch.eye(4, dtype=torch.float64, device="cuda").repeat(S, 1, 1).contiguous()
    cloud = torch.full((S, cap, 3), -7.0, dtype=torch.float32, device="cuda"); edge = cloud.clone()
    cnt = torch.full((S,), -7, dtype=torch.int32, device="cuda"); ecnt = cnt.clone()
    work = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device="cuda")
    d = capi.dptr

    def call(**kw):
        a = dict(depth=d(img), kind=capi.AMK_DEPTH_F32, rows=rows, cols=cols, scene_stride=rows * cols, S=S, Twb=d(T), Twc=d(T),
                 cloud=d(cloud), cloud_stride=cap * 3, cnt=d(cnt), edge=d(edge), edge_stride=cap * 3, ecnt=d(ecnt), stride=3,
                 work=d(work), work_bytes=nbytes.value)
        a.update(kw)
        return lib.amk_depth_to_clouds(a["depth"], a["kind"], a["rows"], a["cols"], a["scene_stride"], a["S"], C.byref(p), a["Twb"], a["Twc"],
                                       a["cloud"], a["cloud_stride"], a["cnt"], a["edge"], a["edge_stride"], a["ecnt"], a["stride"],
                                       a["work"], a["work_bytes"], capi.stream_ptr(None))

    for null in ("depth", "Twb", "Twc", "cloud", "cnt", "edge", "ecnt", "work"):
        assert call(**{null: None}) == capi.AMK_ERR_INVALID_ARG, null
    assert call(work_bytes=nbytes.value - 1) == capi.AMK_ERR_INVALID_ARG
    assert call(scene_stride=rows * cols - 1) == capi.AMK_ERR_INVALID_ARG
    assert call(cloud_stride=cap * 3 - 1) == capi.AMK_ERR_INVALID_ARG
    assert call(edge_stride=cap * 3 - 1) == capi.AMK_ERR_INVALID_ARG
    assert call(S=0) == capi.AMK_ERR_INVALID_ARG and call(stride=2) == capi.AMK_ERR_INVALID_ARG
    assert call(kind=7) == capi.AMK_ERR_UNSUPPORTED
    # a 4 x 2049 image at scale 1: W > AMK_DEPTH_MAX_WIDTH (its buffers fit in the ones above)
    assert call(rows=4, cols=2049, scene_stride=4 * 2049) == capi.AMK_ERR_UNSUPPORTED
    assert call(rows=3, cols=5333, scene_stride=3 * 5333) == capi.AMK_ERR_UNSUPPORTED   # (15 999 pixels: one block's worth, too wide)
    torch.cuda.synchronize()
    for t in (cloud, edge, cnt, ecnt):
        assert bool((t == -7).all())
    # the widest image runs, tiled (8 x 2048 = 16 384 pixels, bands of 4 rows): a flat wall, every pixel kept, no edge
    assert call(rows=8, cols=2048, scene_stride=8 * 2048, S=1) == capi.AMK_OK
    torch.cuda.synchronize()
    assert int(cnt[0]) == 8 * 2048 and int(ecnt[0]) == 0 and int(cnt[1]) == -7 and int(ecnt[1]) == -7
    assert bool((cloud[0, :8 * 2048] != -7).all()) and bool((cloud[0, 8 * 2048:] == -7).all()) and bool((edge == -7).all())


def test_pipeline_depth_frames_above_the_old_limit(torch_cuda):
    """Depth frames of 160 x 120 = 19 200 down-scaled pixels through the pipeline (refused with AMK_ERR_UNSUPPORTED before the tiled
    kernels): every output equals, bit for bit, that of a second pipeline fed the clouds host.depth_to_clouds makes from the same
    images -- the edge clouds with the identity in period 0 and Twb0 * Tbc in period 1, the Twc the slot keeps."""
    torch = torch_cuda
    from avoid_mpc_amd import flight, synth
    from avoid_mpc_amd.host import Pipeline, depth_params, depth_to_clouds
    from tests import _flight
    prm = synth.MpcParams(T=0.33, K=3)
    S, n, periods = 2, 19200, 2
    cam = dict(_flight.DEPTH_CAM, resize_scale=2.0)
    dp = depth_params(cam["pixel2meter"], cam["depth_min"], cam["depth_max"], cam["resize_scale"], cam["fx"], cam["fy"], cam["cx"],
                      cam["cy"], cam["Tbc"])
    dev = torch.device("cuda", torch.cuda.current_device())
    dbl = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    seeds = [11, 12]
    worlds = [flight.FlightWorld(sd, prm, 1000) for sd in seeds]
    st = [flight.initial_state(sd, prm) for sd in seeds]
    x = np.stack([a for a, _ in st]); ref0 = np.stack([b for _, b in st])
    Twc = np.stack([np.eye(4)] * S)
    depth_frames, cloud_frames = [], []
    for t in range(periods):
        fr = [_flight._depth_frame(worlds[i], x[i], cam) for i in range(S)]
        depth = torch.from_numpy(np.stack([d for d, _ in fr]).view(np.int16)).to(dev)
        Twb = np.stack([T for _, T in fr])
        common = dict(odom=dbl(x), ref_path_init=dbl(ref0) if t == 0 else None, keep_warm_start=t > 0)
        depth_frames.append(dict(depth=depth, Twb=dbl(Twb), **common))
        cloud, counts, edge, ecounts = depth_to_clouds(depth, dp, dbl(Twb), dbl(Twc))
        torch.cuda.synchronize()
        assert int(counts.min()) > 0 and int(ecounts.min()) > 10     # (an empty frame would keep an index that was never built)
        cloud_frames.append(dict(clouds=cloud, edges=edge, cloud_counts=counts, edge_counts=ecounts, **common))
        Twc = Twb @ np.asarray(cam["Tbc"])                           # mCurFrame.Twc = mat4Twb * mParamTbc, :50
        x = x.copy(); x[:, 0] += prm.speed * prm.dt

    def run(frames):
        pl = Pipeline(1, S, n, n, prm, queue_depth=1, depth=dp)
        res = []
        for t in range(periods):
            cmd = torch.zeros((S, 3), dtype=torch.float64, device=dev)
            f = dict(frames[t])
            tk = pl.submit(f.pop("clouds", None), f.pop("edges", None), cmd_out=cmd, **f)
            pl.wait(tk)
            o = pl.outputs(tk)
            o["cmd"] = cmd.cpu().numpy()
            res.append(o)
        pl.close()
        return res

    got, want = run(depth_frames), run(cloud_frames)
    for t in range(periods):
        for name in ("u", "x0array", "flags", "ref_path", "cmd"):
            assert np.array_equal(got[t][name], want[t][name]), (t, name)
    assert np.abs(got[0]["cmd"]).max() > 0 and not np.array_equal(got[0]["u"], got[1]["u"])   # (the frames ran, and differ)
