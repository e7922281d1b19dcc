"""cugs_tsdf_integrate / cugs_mesh_workspace_bytes / cugs_mesh_plan / cugs_mesh_emit (include/cugs_hip.h): the workspace
size and every argument check with its place in the order, through ctypes with null or never-dereferenced pointers -
every call here returns before anything is queued.  No GPU."""
import ctypes as C

EINVAL, EALIGN, EOVERFLOW, EWORKSPACE = -1, -2, -3, -4
CHUNK, L2 = 1024, 256                                                     # cells per chunk, chunks per second-level block
inf, nan = float("inf"), float("nan")
BAD_POSITIVE = (0.0, -1.0, inf, nan, -inf)


def _volume(**kw):
    from cugs_amd._lib import TsdfVolume
    kw.setdefault("planes", 0x10000)
    for k, v in (("nx", 8), ("ny", 8), ("nz", 8), ("color", 0), ("voxel_size", 0.1), ("trunc", 0.4)):
        kw.setdefault(k, v)
    return TsdfVolume(**kw)


def _view(**kw):
    from cugs_amd._lib import Camera, TsdfView
    cam = Camera(fx=kw.pop("fx", 50.0), fy=kw.pop("fy", 50.0), cx=8.0, cy=8.0, width=kw.pop("width", 16),
                 height=kw.pop("height", 16))
    kw.setdefault("depth_map", 0x20000)
    kw.setdefault("alpha", 0x30000)
    return TsdfView(camera=cam, **kw)


def _opts(**kw):
    from cugs_amd._lib import TsdfOpts
    for k, v in (("min_depth", 0.05), ("min_alpha", 0.5), ("max_weight", 64.0)):
        kw.setdefault(k, v)
    return TsdfOpts(**kw)


def _round256(b):
    return -(-b // 256) * 256


def _expected_bytes(nx, ny, nz):
    cells = (nx - 1) * (ny - 1) * (nz - 1)
    chunks = -(-cells // CHUNK)
    padded = chunks * CHUNK
    return (2 * _round256(padded) + _round256(4 * padded) + _round256(8 * chunks) + _round256(16 * -(-chunks // L2)) + 256)


def test_mesh_workspace_bytes(pkg):
    from cugs_amd._lib import lib
    size = lib.cugs_mesh_workspace_bytes
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -1, 4), (4, 4, -1)):
        assert size(*bad) == 0
    assert size(2048, 2048, 512) == 0 and size(65536, 65536, 1) == 0           # nx ny nz > 2^31 - 1
    for dims in ((1, 1, 1), (9, 1, 8), (2, 2, 2), (37, 29, 23), (40, 32, 24), (72, 64, 60), (256, 256, 256), (512, 512, 512)):
        assert size(*dims) % 256 == 0
        assert size(*dims) == _expected_bytes(*dims)                           # 6 bytes per padded cell and the scan rows
    assert size(1, 1, 1) == size(9, 1, 8) == 256                               # no cells: the totals alone
    assert size(2, 2, 2) == size(11, 11, 11)                                   # 1 and 1000 cells: one chunk
    assert size(11, 11, 11) < size(12, 11, 11)                                 # 1100 cells: two
    assert size(37, 29, 23) < size(72, 64, 60) < size(256, 256, 256)
    assert size(1290, 1290, 1290) > 0                                          # just under 2^31 voxels


def test_tsdf_integrate_argument_validation(pkg):
    from cugs_amd._lib import TsdfView, lib
    null = C.c_void_p(0)

    def call(vol=None, views=None, n=None, opts=None, **kw):
        vol = _volume() if vol is None else vol
        views = [_view()] if views is None else views
        table = (TsdfView * max(len(views), 1))(*views)
        return lib.cugs_tsdf_integrate(kw.get("vol_p", C.byref(vol)), kw.get("views_p", table), len(views) if n is None else n,
                                       kw.get("opts_p", C.byref(_opts() if opts is None else opts)), null)

    assert call(vol_p=None) == EINVAL and call(views_p=None) == EINVAL and call(opts_p=None) == EINVAL
    for k in ("nx", "ny", "nz"):
        for bad in (0, -1):
            assert call(_volume(**{k: bad})) == EINVAL
    for n in (0, -1, 17, 1 << 20):
        assert call(views=[_view()] * 16, n=n) == EINVAL                       # num_views outside 1..16
    assert call(_volume(planes=0)) == EINVAL
    for bad in BAD_POSITIVE:
        assert call(_volume(voxel_size=bad)) == EINVAL
        assert call(_volume(trunc=bad)) == EINVAL
        for k in ("min_depth", "min_alpha", "max_weight"):
            assert call(opts=_opts(**{k: bad})) == EINVAL
        assert call(views=[_view(), _view(fx=bad)]) == EINVAL                  # every view of the table is checked
        assert call(views=[_view(), _view(fy=bad)]) == EINVAL
    for bad in (0, -1):
        assert call(views=[_view(width=bad)]) == EINVAL
        assert call(views=[_view(), _view(), _view(height=bad)]) == EINVAL
    assert call(views=[_view(depth_map=0)]) == EINVAL
    assert call(views=[_view(alpha=0)]) == EINVAL
    assert call(_volume(color=1), views=[_view(color=0x40000), _view()]) == EINVAL   # colour planes, a view without colour
    # views past num_views are not looked at
    assert call(_volume(nx=2048, ny=2048, nz=512), views=[_view(), _view(fx=0.0)], n=1) == EOVERFLOW
    # the order: every CUGS_EINVAL comes before CUGS_EOVERFLOW
    big = dict(nx=2048, ny=2048, nz=512)
    assert call(_volume(**big)) == EOVERFLOW
    assert call(_volume(nx=65536, ny=65536, nz=1)) == EOVERFLOW
    assert call(_volume(**big), views=[_view(weight=0x50000)]) == EOVERFLOW         # the optional maps change nothing
    assert call(_volume(color=1, **big), views=[_view(color=0x40000)]) == EOVERFLOW
    assert call(_volume(planes=0, **big)) == EINVAL
    assert call(_volume(trunc=0.0, **big)) == EINVAL
    assert call(_volume(**big), opts=_opts(min_alpha=nan)) == EINVAL
    assert call(_volume(**big), views=[_view(fx=inf)]) == EINVAL
    assert call(_volume(**big), views=[_view(alpha=0)]) == EINVAL
    assert call(_volume(color=1, **big)) == EINVAL
    assert call(_volume(**big), n=17) == EINVAL


def test_mesh_plan_argument_validation(pkg):
    from cugs_amd._lib import lib
    null, ws = C.c_void_p(0), C.c_void_p(0x100000)
    counts = (C.c_int64 * 2)(7, 7)
    need = lib.cugs_mesh_workspace_bytes(8, 8, 8)

    def call(vol, min_weight=0.0, w=ws, wb=1 << 30, c=counts):
        return lib.cugs_mesh_plan(C.byref(vol) if vol is not None else None, min_weight, w, wb, c, null)

    assert call(None) == EINVAL
    for k in ("nx", "ny", "nz"):
        for bad in (0, -1):
            assert call(_volume(**{k: bad})) == EINVAL
    assert call(_volume(planes=0)) == EINVAL
    for bad in BAD_POSITIVE:
        assert call(_volume(voxel_size=bad)) == EINVAL
        assert call(_volume(trunc=bad)) == EINVAL
    for bad in (-1e-3, inf, nan, -inf):
        assert call(_volume(), min_weight=bad) == EINVAL
    assert call(_volume(), w=null) == EINVAL
    assert call(_volume(), c=None) == EINVAL
    assert call(_volume(), wb=0) == EWORKSPACE and call(_volume(), wb=need - 1) == EWORKSPACE
    assert call(_volume(), w=C.c_void_p(0x100004), wb=need) == EALIGN
    assert call(_volume(nx=2048, ny=2048, nz=512)) == EOVERFLOW
    # the order: CUGS_EINVAL, then CUGS_EOVERFLOW, then CUGS_EWORKSPACE, then CUGS_EALIGN
    assert call(_volume(nx=2048, ny=2048, nz=512), min_weight=nan, wb=0) == EINVAL
    assert call(_volume(nx=2048, ny=2048, nz=512), wb=0, w=C.c_void_p(0x100004)) == EOVERFLOW
    assert call(_volume(), wb=0, w=C.c_void_p(0x100004)) == EWORKSPACE
    assert call(_volume(trunc=0.0), wb=0) == EINVAL
    # a box one voxel thin has no cells: {0, 0}, nothing queued
    assert call(_volume(ny=1), wb=256) == 0
    assert list(counts) == [0, 0]


def test_mesh_emit_argument_validation(pkg):
    from cugs_amd._lib import lib
    null, ws = C.c_void_p(0), C.c_void_p(0x100000)
    v, c, f = C.c_void_p(0x200000), C.c_void_p(0x300000), C.c_void_p(0x400000)
    need = lib.cugs_mesh_workspace_bytes(8, 8, 8)

    def call(vol, nv=10, nf=20, w=ws, wb=1 << 30, V=v, Cc=null, F=f):
        return lib.cugs_mesh_emit(C.byref(vol) if vol is not None else None, w, wb, nv, nf, V, Cc, F, null)

    assert call(None) == EINVAL
    for k in ("nx", "ny", "nz"):
        for bad in (0, -1):
            assert call(_volume(**{k: bad})) == EINVAL
    assert call(_volume(planes=0)) == EINVAL
    for bad in BAD_POSITIVE:
        assert call(_volume(voxel_size=bad)) == EINVAL
        assert call(_volume(trunc=bad)) == EINVAL
    assert call(_volume(), w=null) == EINVAL
    assert call(_volume(), nv=-1) == EINVAL and call(_volume(), nf=-1) == EINVAL
    assert call(_volume(), V=null) == EINVAL and call(_volume(), F=null) == EINVAL
    assert call(_volume(), Cc=c) == EINVAL                                      # colours from a volume without colour
    assert call(_volume(), wb=0) == EWORKSPACE and call(_volume(), wb=need - 1) == EWORKSPACE
    assert call(_volume(), w=C.c_void_p(0x100008), wb=need) == EALIGN
    assert call(_volume(), nv=7 * 7 * 7 + 1) == EINVAL                          # more vertices than cells
    assert call(_volume(), nf=6 * 7 * 7 * 7 + 1) == EINVAL
    assert call(_volume(nx=2048, ny=2048, nz=512)) == EOVERFLOW
    # the order
    assert call(_volume(nx=2048, ny=2048, nz=512), nv=-1, wb=0) == EINVAL
    assert call(_volume(nx=2048, ny=2048, nz=512), wb=0) == EOVERFLOW
    assert call(_volume(), wb=0, w=C.c_void_p(0x100008)) == EWORKSPACE
    assert call(_volume(), nv=7 * 7 * 7 + 1, wb=0) == EWORKSPACE                # the counts are judged last
    assert call(_volume(), nv=7 * 7 * 7 + 1, wb=need, w=C.c_void_p(0x100008)) == EALIGN
    # zero counts queue nothing, with or without output arrays
    assert call(_volume(), nv=0, nf=0, V=null, F=null, wb=need) == 0
    assert call(_volume(color=1), nv=0, nf=0, Cc=c, wb=need) == 0
