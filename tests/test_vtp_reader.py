"""The VTK-free .vtp reader (csrc/host/vtp_reader.cpp, dmi_read_polydata): the files this project writes round-trip bit for
bit, every data mode of the format is read, and what the reader does not take is refused with a reason.  No GPU."""
import itertools

import numpy as np
import pytest

from cudadepthmapintegration_amd import capi
from vtp_writer import write_vtp


def _mesh(seed=0, n=40, m=60):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((n, 3))
    pts[0] = [np.pi, -0.0, 1e-300]
    tris = rng.integers(0, n, size=(m, 3))
    return pts, tris


def test_write_polydata_round_trips_bit_for_bit(tmp_path):
    pts, tris = _mesh()
    capi.write_polydata(str(tmp_path / "m.vtp"), pts, tris)
    r = capi.read_polydata(str(tmp_path / "m.vtp"))
    assert r.points.dtype == np.float64 and r.points.tobytes() == pts.tobytes()
    assert r.connectivity.dtype == np.int64 and np.array_equal(r.connectivity, tris.reshape(-1))
    assert np.array_equal(r.offsets, 3 * np.arange(1, len(tris) + 1))
    assert r.point_data == {} and r.cell_data == {} and r.point_designations == [] and r.cell_designations == []
    capi.write_polydata(str(tmp_path / "e.vtp"), np.zeros((0, 3)), np.zeros((0, 3), np.int64))   # an empty mesh
    e = capi.read_polydata(str(tmp_path / "e.vtp"))
    assert e.points.shape == (0, 3) and e.connectivity.size == 0 and e.offsets.size == 0


def test_write_polydata_with_normals_round_trips_bit_for_bit(tmp_path):
    pts, tris = _mesh(1)
    normals = np.random.default_rng(2).standard_normal((len(pts), 3)).astype(np.float32)
    capi.write_polydata_with_normals(str(tmp_path / "n.vtp"), pts, tris, normals, 0.25)
    r = capi.read_polydata(str(tmp_path / "n.vtp"))
    assert r.points.tobytes() == pts.tobytes() and np.array_equal(r.connectivity, tris.reshape(-1))
    assert list(r.point_data) == ["Normals", "reconstruction_scalar"]
    assert r.point_data["Normals"].dtype == np.float32 and r.point_data["Normals"].tobytes() == normals.tobytes()
    assert r.point_data["reconstruction_scalar"].dtype == np.float64 and np.all(r.point_data["reconstruction_scalar"] == 0.25)
    assert r.point_designations == [("Normals", "Normals"), ("Scalars", "reconstruction_scalar")]


MODES = ["ascii", "binary", "appended-raw", "appended-base64"]


@pytest.mark.parametrize("mode,compress,header,big_endian", [
    (m, c, h, b) for m, c, h, b in itertools.product(MODES, (False, True), ("UInt32", "UInt64"), (False, True))
    if not (m == "ascii" and c)])                      # (ascii text is never compressed)
@pytest.mark.parametrize("pdt,idt", list(itertools.product((np.float32, np.float64), (np.int32, np.int64))))
def test_every_data_mode(tmp_path, mode, compress, header, big_endian, pdt, idt):
    rng = np.random.default_rng(7)
    n = 50
    pts = rng.standard_normal((n, 3)).astype(pdt)
    sizes = rng.integers(3, 7, size=23)                                # polygons of any size
    offsets = np.cumsum(sizes).astype(idt)
    conn = rng.integers(0, n, size=int(offsets[-1])).astype(idt)
    pd = {"Normals": rng.standard_normal((n, 3)).astype(np.float32), "label": rng.integers(-5, 5, n).astype(np.int16),
          "wide": rng.integers(0, 2 ** 40, (n, 2)).astype(np.uint64)}
    cd = {"cell_id": np.arange(len(sizes), dtype=np.int32), "rgb": rng.integers(0, 255, (len(sizes), 3)).astype(np.uint8)}
    path = str(tmp_path / "x.vtp")
    write_vtp(path, pts, conn, offsets, pd, cd, mode=mode, compress=compress, header=header, big_endian=big_endian, block=64,
              point_attrs='Normals="Normals" Scalars="label"', cell_attrs='Scalars="cell_id"')
    r = capi.read_polydata(path)
    assert r.points.dtype == pdt and r.points.tobytes() == pts.tobytes()
    assert r.connectivity.dtype == idt and np.array_equal(r.connectivity, conn)
    assert r.offsets.dtype == idt and np.array_equal(r.offsets, offsets)
    assert list(r.point_data) == list(pd) and list(r.cell_data) == list(cd)
    for k, v in pd.items():
        assert r.point_data[k].dtype == v.dtype and r.point_data[k].tobytes() == v.tobytes(), k
    for k, v in cd.items():
        assert r.cell_data[k].dtype == v.dtype and r.cell_data[k].tobytes() == v.tobytes(), k
    assert r.point_designations == [("Normals", "Normals"), ("Scalars", "label")]
    assert r.cell_designations == [("Scalars", "cell_id")]


def _refused(tmp_path, needle, **kw):
    pts = np.zeros((4, 3))
    args = dict(connectivity=np.array([0, 1, 2, 1, 2, 3], np.int64), offsets=np.array([3, 6], np.int64))
    args.update({k: kw.pop(k) for k in list(kw) if k in args})
    path = str(tmp_path / "bad.vtp")
    write_vtp(path, pts, args["connectivity"], args["offsets"], **kw)
    with pytest.raises(ValueError) as e:
        capi.read_polydata(path)
    assert needle in str(e.value), str(e.value)


@pytest.mark.parametrize("kw,needle", [
    (dict(piece_extra='NumberOfVerts="1"'), "Verts, Lines or Strips"),
    (dict(piece_extra='NumberOfLines="2"'), "Verts, Lines or Strips"),
    (dict(piece_extra='NumberOfStrips="1"'), "Verts, Lines or Strips"),
    (dict(extra_pieces=1), "more than one <Piece>"),
    (dict(with_points=False), "no <Points>"),
    (dict(offsets=np.array([3, 3], np.int64)), "not increasing"),
    (dict(offsets=np.array([4, 2], np.int64)), "not increasing"),
    (dict(offsets=np.array([3, 7], np.int64)), "overrun the connectivity"),
    (dict(connectivity=np.array([0, 1, 2, 1, 2, 4], np.int64)), "out of range"),
    (dict(connectivity=np.array([0, 1, -1, 1, 2, 3], np.int64)), "out of range"),
    (dict(compress=True, compressor="vtkLZ4DataCompressor"), "unsupported compressor"),
    (dict(compress=True, compressor="vtkLZMADataCompressor"), "unsupported compressor"),
])
def test_refusals(tmp_path, kw, needle):
    _refused(tmp_path, needle, **kw)


def test_not_polydata_and_missing_file(tmp_path):
    with pytest.raises(ValueError, match="cannot open"):
        capi.read_polydata(str(tmp_path / "none.vtp"))
    (tmp_path / "img.vtp").write_text('<?xml version="1.0"?>\n<VTKFile type="ImageData"><ImageData/></VTKFile>\n')
    with pytest.raises(ValueError, match="not PolyData"):
        capi.read_polydata(str(tmp_path / "img.vtp"))
