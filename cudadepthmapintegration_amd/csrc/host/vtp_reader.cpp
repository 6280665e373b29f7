// vtp_reader.cpp -- see vtp_reader.h.
#include "vtp_reader.h"

#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <sstream>

namespace dmi {
namespace host {
namespace vtp {

namespace {

using vtkxml::Attr;
using vtkxml::Fail;

int64_t integer_at(const Array &a, int64_t i) {
  if (a.elem_size == 4) {
    int32_t v;
    std::memcpy(&v, a.bytes.data() + 4 * (size_t)i, 4);
    return v;
  }
  int64_t v;
  std::memcpy(&v, a.bytes.data() + 8 * (size_t)i, 8);
  return v;
}

// [begin, end) of the section <name ...> ... </name> inside the piece (*tag = its opening tag's text); false: absent
bool section(const std::string &text, const std::string &name, size_t from, size_t to, size_t *begin, size_t *end,
             std::string *tag, bool *empty) {
  size_t p = from;
  for (;;) {
    p = text.find("<" + name, p);
    if (p == std::string::npos || p >= to) return false;
    const char c = text[p + 1 + name.size()];
    if (c == ' ' || c == '>' || c == '/' || c == '\t' || c == '\n' || c == '\r') break;
    ++p;
  }
  const size_t tag_end = text.find('>', p);
  if (tag_end == std::string::npos || tag_end > to) return false;
  *tag = text.substr(p, tag_end - p);
  *begin = tag_end + 1;
  *empty = text[tag_end - 1] == '/';
  if (*empty) {
    *end = *begin;
    return true;
  }
  const size_t close = text.find("</" + name + ">", tag_end);
  *end = close == std::string::npos || close > to ? std::string::npos : close;
  return true;
}

// every <DataArray> in text[begin, end)
bool arrays_in(const std::string &text, size_t begin, size_t end, const vtkxml::Appended &app, const vtkxml::Format &fmt,
               int64_t n_tuples, const std::string &path, const std::string &where, std::vector<Array> *out, std::string *err) {
  size_t p = begin;
  while ((p = text.find("<DataArray", p)) != std::string::npos && p < end) {
    const size_t tag_end = text.find('>', p);
    if (tag_end == std::string::npos || tag_end > end) return Fail(err, path + ": malformed <DataArray> in " + where);
    const bool self_closed = text[tag_end - 1] == '/';
    const std::string tag = text.substr(p, tag_end - p);
    p = tag_end + 1;
    Array a;
    std::string s;
    Attr(tag, "Name", &a.name);
    if (!Attr(tag, "type", &a.type) || (a.elem_size = vtkxml::TypeSize(a.type)) == 0)
      return Fail(err, path + ": array '" + a.name + "' in " + where + " has an unknown type");
    if (Attr(tag, "NumberOfComponents", &s)) a.components = std::atoi(s.c_str());
    if (a.components < 1 || a.components > 1024)
      return Fail(err, path + ": array '" + a.name + "' in " + where + " has an impossible component count");
    if (!vtkxml::DecodeDataArray(text, tag, self_closed, p, end, app, fmt, (size_t)n_tuples, path, &a, &p, err)) return false;
    out->push_back(std::move(a));
  }
  return true;
}

bool count_attr(const std::string &tag, const char *name, int64_t *out) {
  std::string s;
  *out = 0;
  if (!Attr(tag, name, &s)) return true;  // absent: none
  char *end = nullptr;
  const long long v = std::strtoll(s.c_str(), &end, 10);
  if (end == s.c_str() || v < 0) return false;
  *out = v;
  return true;
}

bool read_poly_data(const std::string &path, PolyData *out, std::string *err) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f.is_open()) return Fail(err, "cannot open " + path);
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string text = ss.str();

  const size_t vf = text.find("<VTKFile");
  if (vf == std::string::npos) return Fail(err, path + ": not a VTK XML file");
  const std::string vtag = text.substr(vf, text.find('>', vf) - vf);
  std::string s;
  if (!Attr(vtag, "type", &s) || s != "PolyData") return Fail(err, path + ": VTKFile type is not PolyData");
  vtkxml::Format fmt;
  if (!vtkxml::ReadFormat(vtag, path, &fmt, err)) return false;
  const size_t pd = text.find("<PolyData", vf);
  if (pd == std::string::npos) return Fail(err, path + ": no <PolyData> element");
  vtkxml::Appended app;
  size_t xml_end = text.size();
  if (!vtkxml::FindAppended(text, pd, path, &app, &xml_end, err)) return false;

  const size_t piece = text.find("<Piece", pd);
  if (piece == std::string::npos || piece >= xml_end) return Fail(err, path + ": no <Piece> element");
  const size_t piece_end = text.find("</Piece>", piece);
  if (piece_end == std::string::npos || piece_end > xml_end) return Fail(err, path + ": unterminated <Piece>");
  if (text.find("<Piece", piece_end) < xml_end) return Fail(err, path + ": more than one <Piece> (only single-piece files are read)");
  const std::string ptag = text.substr(piece, text.find('>', piece) - piece);
  int64_t nverts = 0, nlines = 0, nstrips = 0;
  if (!count_attr(ptag, "NumberOfPoints", &out->n_points) || !count_attr(ptag, "NumberOfPolys", &out->n_polys) ||
      !count_attr(ptag, "NumberOfVerts", &nverts) || !count_attr(ptag, "NumberOfLines", &nlines) ||
      !count_attr(ptag, "NumberOfStrips", &nstrips))
    return Fail(err, path + ": malformed counts in <Piece>");
  if (nverts || nlines || nstrips)
    return Fail(err, path + ": the piece has Verts, Lines or Strips (only Polys are read)");
  if (out->n_points > (int64_t(1) << 40) || out->n_polys > (int64_t(1) << 40)) return Fail(err, path + ": counts too large");

  size_t b = 0, e = 0;
  std::string tag;
  bool empty = false;
  // Points
  std::vector<Array> pts;
  if (!section(text, "Points", piece, piece_end, &b, &e, &tag, &empty) || e == std::string::npos)
    return Fail(err, path + ": no <Points> element");
  if (!arrays_in(text, b, e, app, fmt, out->n_points, path, "<Points>", &pts, err)) return false;
  if (pts.empty()) return Fail(err, path + ": <Points> holds no array");
  if (pts.size() != 1 || pts[0].components != 3 || (pts[0].type != "Float32" && pts[0].type != "Float64"))
    return Fail(err, path + ": Points must be one Float32 or Float64 array of 3 components");
  out->points = std::move(pts[0]);
  // Polys: connectivity and offsets, read in two steps (offsets first: they give the connectivity's length)
  out->connectivity = Array();
  out->offsets = Array();
  out->connectivity.type = out->offsets.type = "Int64";
  out->connectivity.elem_size = out->offsets.elem_size = 8;
  if (out->n_polys > 0) {
    if (!section(text, "Polys", piece, piece_end, &b, &e, &tag, &empty) || e == std::string::npos)
      return Fail(err, path + ": NumberOfPolys > 0 without a <Polys> element");
    size_t conn_at = std::string::npos, off_at = std::string::npos;
    for (size_t p = b; (p = text.find("<DataArray", p)) != std::string::npos && p < e; ++p) {
      const std::string t = text.substr(p, text.find('>', p) - p);
      std::string name;
      Attr(t, "Name", &name);
      if (name == "connectivity") conn_at = p;
      if (name == "offsets") off_at = p;
    }
    if (conn_at == std::string::npos || off_at == std::string::npos)
      return Fail(err, path + ": <Polys> without connectivity and offsets arrays");
    auto one = [&](size_t at, int64_t n, Array *dst) {
      const size_t te = text.find('>', at);
      std::vector<Array> got;
      // (the single array's tag through arrays_in: it stops at the tag's own end)
      const size_t close = text[te - 1] == '/' ? te + 1 : text.find("</DataArray>", te);
      if (close == std::string::npos || close > e) return Fail(err, path + ": unterminated <DataArray> in <Polys>");
      if (!arrays_in(text, at, close + 1, app, fmt, n, path, "<Polys>", &got, err)) return false;
      if (got.size() != 1 || got[0].components != 1 || (got[0].type != "Int32" && got[0].type != "Int64"))
        return Fail(err, path + ": Polys' " + (dst == &out->offsets ? "offsets" : "connectivity") + " must be one Int32 or Int64 array");
      *dst = std::move(got[0]);
      return true;
    };
    if (!one(off_at, out->n_polys, &out->offsets)) return false;
    // offsets: increasing, the last one the connectivity's length
    int64_t prev = 0;
    for (int64_t i = 0; i < out->n_polys; ++i) {
      const int64_t o = out->OffsetAt(i);
      if (o <= prev) return Fail(err, path + ": Polys offsets are not increasing");
      prev = o;
    }
    // the connectivity holds exactly what the last offset calls for: one of another length is refused by its decoding
    if (prev > (int64_t(1) << 44) || !one(conn_at, prev, &out->connectivity))
      return Fail(err, path + ": Polys offsets overrun the connectivity (the last offset is " + std::to_string(prev) + "): " +
                           (err ? *err : std::string()));
    for (int64_t i = 0; i < prev; ++i) {
      const int64_t id = out->ConnectivityAt(i);
      if (id < 0 || id >= out->n_points) return Fail(err, path + ": Polys connectivity id " + std::to_string(id) + " is out of range");
    }
  }
  // PointData / CellData
  out->point_data.clear();
  out->cell_data.clear();
  out->point_designations.clear();
  out->cell_designations.clear();
  if (section(text, "PointData", piece, piece_end, &b, &e, &tag, &empty)) {
    if (e == std::string::npos) return Fail(err, path + ": unterminated <PointData>");
    out->point_designations = vtkxml::Attributes(tag);
    if (!arrays_in(text, b, e, app, fmt, out->n_points, path, "<PointData>", &out->point_data, err)) return false;
  }
  if (section(text, "CellData", piece, piece_end, &b, &e, &tag, &empty)) {
    if (e == std::string::npos) return Fail(err, path + ": unterminated <CellData>");
    out->cell_designations = vtkxml::Attributes(tag);
    if (!arrays_in(text, b, e, app, fmt, out->n_polys, path, "<CellData>", &out->cell_data, err)) return false;
  }
  return true;
}

}  // namespace

int64_t PolyData::ConnectivityAt(int64_t i) const { return integer_at(connectivity, i); }
int64_t PolyData::OffsetAt(int64_t i) const { return integer_at(offsets, i); }

bool ReadPolyData(const std::string &path, PolyData *out, std::string *err) {
  // nothing thrown by the containers may leave this function: its callers sit right below extern "C" entry points
  try {
    return read_poly_data(path, out, err);
  } catch (const std::exception &e) {
    return Fail(err, path + ": " + e.what());
  } catch (...) {
    return Fail(err, path + ": unknown failure while reading");
  }
}

}  // namespace vtp
}  // namespace host
}  // namespace dmi
