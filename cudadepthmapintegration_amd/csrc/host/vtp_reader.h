// vtp_reader.h -- VTK-free reader for VTK XML PolyData (.vtp): what the reference's Coloration tool reads with
// vtkXMLPolyDataReader (Coloration/main.cxx:75-77) before colouring the mesh.
//
// One <Piece>; <Points> (Float32 or Float64, 3 components); <Polys> with Int32 or Int64 connectivity and offsets, polygons of
// any size; every <PointData> and <CellData> array of any numeric type and component count, kept byte for byte with the
// attribute designations of its section (Normals="Normals" Scalars="..." ...).  Every data mode of the format (ascii, binary,
// appended raw / base64, zlib or not, UInt32 / UInt64 headers, either byte order) through the decoding the .vti reader uses
// (vtk_xml_data.h).  Refused with a message: non-empty Verts, Lines or Strips, more than one piece, no Points array, offsets
// that are not increasing or overrun the connectivity, connectivity ids out of range, LZ4 / LZMA compressors.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "vtk_xml_data.h"

namespace dmi {
namespace host {
namespace vtp {

using Array = vtkxml::Array;

struct PolyData {
  int64_t n_points = 0, n_polys = 0;
  Array points;                     // "Points": Float32 or Float64 x 3, n_points tuples
  Array connectivity, offsets;      // "Polys": Int32 or Int64 each; offsets[i] = end of polygon i in connectivity
  std::vector<Array> point_data, cell_data;  // in file order
  // the attributes of <PointData ...> / <CellData ...>: the designations (Scalars="name", Normals="name", ...)
  std::vector<std::pair<std::string, std::string>> point_designations, cell_designations;
  int64_t ConnectivityAt(int64_t i) const;  // as int64 whatever the stored type
  int64_t OffsetAt(int64_t i) const;
};

// false + *err on any malformed, unsupported or refused content; nothing is printed.
bool ReadPolyData(const std::string &path, PolyData *out, std::string *err);

}  // namespace vtp
}  // namespace host
}  // namespace dmi
