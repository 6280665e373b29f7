"""Test utility: writes VTK XML PolyData (.vtp) files in every data mode of the format, from its published description (not
from VTK code): ascii, inline binary (base64), appended raw / base64, with or without the zlib compressor, UInt32 / UInt64
headers, little / big endian; Float32 / Float64 points, Int32 / Int64 connectivity and offsets, point and cell arrays of any
type.  Used to exercise host/vtp_reader.cpp; the payload encoding is vti_writer's."""
import numpy as np

from vti_writer import _payload

_TYPES = {np.dtype("float64"): "Float64", np.dtype("float32"): "Float32", np.dtype("uint8"): "UInt8", np.dtype("int8"): "Int8",
          np.dtype("int16"): "Int16", np.dtype("uint16"): "UInt16", np.dtype("int32"): "Int32", np.dtype("uint32"): "UInt32",
          np.dtype("int64"): "Int64", np.dtype("uint64"): "UInt64"}


def write_vtp(path, points, connectivity, offsets, point_data=None, cell_data=None, mode="appended-raw", compress=False,
              header="UInt64", big_endian=False, block=4096, point_attrs="", cell_attrs="", piece_extra="", extra_pieces=0,
              compressor="vtkZLibDataCompressor", with_points=True):
    """point_data / cell_data: dict name -> array [n] or [n, C].  *_attrs: the designations written into <PointData ...> /
    <CellData ...> as they are (e.g. 'Normals="Normals"').  piece_extra: more attributes of <Piece> (e.g. NumberOfVerts="1").
    mode: ascii | binary | appended-raw | appended-base64."""
    endian = ">" if big_endian else "<"
    attrs = f'type="PolyData" version="{"1.0" if header == "UInt64" else "0.1"}" byte_order="{"BigEndian" if big_endian else "LittleEndian"}"'
    if header == "UInt64":
        attrs += ' header_type="UInt64"'
    if compress:
        attrs += f' compressor="{compressor}"'
    appended = []
    offset = [0]

    def data_array(name, a):
        a = np.ascontiguousarray(a)
        comps = a.shape[1] if a.ndim == 2 else 1
        tag = f'          <DataArray type="{_TYPES[a.dtype]}" Name="{name}" NumberOfComponents="{comps}" '
        raw = a.astype(a.dtype.newbyteorder(endian)).tobytes()
        if mode == "ascii":
            vals = " ".join(repr(float(v)) if a.dtype.kind == "f" else str(int(v)) for v in a.reshape(-1))
            return (tag + 'format="ascii">\n            ' + vals + "\n          </DataArray>\n").encode()
        if mode == "binary":
            return ((tag + 'format="binary">\n            ').encode() + _payload(raw, header, endian, compress, block, True)
                    + b"\n          </DataArray>\n")
        p = _payload(raw, header, endian, compress, block, mode == "appended-base64")
        appended.append(p)
        out = (tag + f'format="appended" offset="{offset[0]}"/>\n').encode()
        offset[0] += len(p)
        return out

    pts = np.asarray(points)
    n_polys = len(offsets)

    def piece():
        others = " ".join(f'NumberOf{c}="0"' for c in ("Verts", "Lines", "Strips") if f"NumberOf{c}" not in piece_extra)
        body = [f'    <Piece NumberOfPoints="{pts.shape[0]}" {others} NumberOfPolys="{n_polys}" {piece_extra}>\n'.encode()]
        body.append(f"      <PointData {point_attrs}>\n".encode())
        for k, v in (point_data or {}).items():
            body.append(data_array(k, v))
        body.append(b"      </PointData>\n")
        body.append(f"      <CellData {cell_attrs}>\n".encode())
        for k, v in (cell_data or {}).items():
            body.append(data_array(k, v))
        body.append(b"      </CellData>\n")
        if with_points:
            body.append(b"      <Points>\n" + data_array("Points", pts) + b"      </Points>\n")
        for cells in ("Verts", "Lines", "Strips"):
            body.append(f"      <{cells}>\n".encode() + data_array("connectivity", np.zeros(0, np.int64))
                        + data_array("offsets", np.zeros(0, np.int64)) + f"      </{cells}>\n".encode())
        body.append(b"      <Polys>\n" + data_array("connectivity", np.asarray(connectivity))
                    + data_array("offsets", np.asarray(offsets)) + b"      </Polys>\n    </Piece>\n")
        return b"".join(body)

    out = [b'<?xml version="1.0"?>\n', f"<VTKFile {attrs}>\n".encode(), b"  <PolyData>\n"]
    for _ in range(1 + extra_pieces):
        out.append(piece())
    out.append(b"  </PolyData>\n")
    if appended:
        enc = "base64" if mode == "appended-base64" else "raw"
        out.append(f'  <AppendedData encoding="{enc}">\n   _'.encode() + b"".join(appended) + b"\n  </AppendedData>\n")
    out.append(b"</VTKFile>\n")
    with open(path, "wb") as f:
        f.write(b"".join(out))
