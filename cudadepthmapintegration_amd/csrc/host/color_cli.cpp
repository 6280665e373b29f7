// color_cli.cpp -- see color_cli.h.  Reference: Coloration/main.cxx ("cmain").
#include "color_cli.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <ostream>
#include <sstream>
#include <vector>

#include "fan_triangulate.h"
#include "recon_host.h"

namespace dmi {
namespace host {
namespace color_cli {

namespace {

struct Flag {
  const char *name;
  bool takes_value;
  const char *help;
};

// cmain:111-116 in the reference's order, then the two flags this tool adds
const Flag kFlags[] = {
    {"--input", true, "(required) Path to a .vtp file"},
    {"--output", true, "(required) Path of the output file (.vtp)"},
    {"--krtd", true, "(required) Path to the file which contains all krtd path"},
    {"--vti", true, "(required) Path to the file which contains all vti path"},
    {"--verbose", false, "(optional) Use to display debug information"},
    {"--help", false, "Print help message"},
    {"--device", true, "(optional, not in the reference) HIP device ordinal (default 0)"},
    {"--depthTolerance", true,
     "(optional, not in the reference) turn on the visibility test: a view adds its pixel to a vertex only if the vertex is in "
     "front of the camera and its camera z is within this distance of the view's 'Depths' value there (finite, >= 0). "
     "Without it the three arrays are the reference's"},
    {"--depthFromMesh", false,
     "(optional, not in the reference; needs --depthTolerance) the visibility test compares against the input mesh's own depth, "
     "rendered into every view on the GPU, instead of the views' 'Depths' arrays (which are then not read and need not exist: "
     "a .vti file with a 'Color' array alone will do): no holes, no noise, "
     "and a mesh from anywhere can be tested.  Polygons of more than three corners are fan-triangulated from their first corner "
     "for the rendering only; a triangle that crosses a camera's plane does not occlude (no near-plane clipping)"},
};

}  // namespace

std::string HelpText() {
  std::ostringstream out;
  out << "dmi_coloration: colours the vertices of a mesh (.vtp) from the views' 'Color' arrays on an MI355X and writes the mesh "
         "with the point arrays MeanColoration, MedianColoration and NbProjectedDepthMap.\n"
         "Unlike the reference, a failed colouring is an error: the tool prints it and exits with status 1.\n";
  for (const Flag &f : kFlags) out << "  " << f.name << (f.takes_value ? " v" : "") << "\n      " << f.help << "\n";
  return out.str();
}

bool ReadArguments(int argc, const char *const *argv, Options *o, std::ostream &err) {
  bool help = false;
  for (int i = 1; i < argc; ++i) {
    const std::string flag = argv[i];
    const Flag *hit = nullptr;
    for (const Flag &f : kFlags)
      if (flag == f.name) hit = &f;
    if (!hit) {  // vtksys's parser fails on an argument nobody registered (cmain:118-123)
      err << "Unknown argument: " << flag << "\n" << HelpText();
      return false;
    }
    if (!hit->takes_value) {
      (flag == "--help" ? help : flag == "--depthFromMesh" ? o->depthFromMesh : o->verbose) = true;
      continue;
    }
    if (i + 1 >= argc) {
      err << flag << " needs a value\n" << HelpText();
      return false;
    }
    const std::string value = argv[++i];
    if (flag == "--input") o->input = value;
    else if (flag == "--output") o->output = value;
    else if (flag == "--krtd") o->krtd = value;
    else if (flag == "--vti") o->vti = value;
    else if (flag == "--device") {
      char *end = nullptr;
      const long d = std::strtol(value.c_str(), &end, 10);
      if (value.empty() || *end || d < 0 || d > 1024) {
        err << "Bad value for --device\n" << HelpText();
        return false;
      }
      o->device = (int)d;
    } else {  // --depthTolerance
      char *end = nullptr;
      const double t = std::strtod(value.c_str(), &end);
      if (value.empty() || *end) {
        err << "Bad value for --depthTolerance\n" << HelpText();
        return false;
      }
      if (!(t >= 0.0 && std::isfinite(t))) {
        err << "Error : --depthTolerance must be a finite number >= 0 (got " << value << ")\n" << HelpText();
        return false;
      }
      o->depthTest = true;
      o->depthTolerance = t;
    }
  }
  if (help) {  // cmain:119-123
    err << HelpText();
    return false;
  }
  if (o->input.empty() || o->output.empty() || o->krtd.empty() || o->vti.empty()) {  // cmain:126-132
    err << "Missing arguments..." << std::endl << HelpText();
    return false;
  }
  if (o->depthFromMesh && !o->depthTest) {
    err << "Error : --depthFromMesh needs --depthTolerance (the rendered depth is what the visibility test compares against)\n" << HelpText();
    return false;
  }
  return true;
}

bool WriteColoredPolyData(const std::string &path, const vtp::PolyData &mesh, const uint8_t *mean, const uint8_t *median,
                          const int32_t *count, std::string *error) {
  const size_t np = (size_t)mesh.n_points;
  // the point arrays after AddArray: the input's, a same-named one replaced where it stood, the others appended
  std::vector<vtp::Array> point_data = mesh.point_data;
  auto add = [&](const char *name, const char *type, int comps, size_t elem, const void *data) {
    vtp::Array a;
    a.name = name;
    a.type = type;
    a.components = comps;
    a.elem_size = elem;
    a.bytes.assign((const unsigned char *)data, (const unsigned char *)data + np * comps * elem);
    for (vtp::Array &b : point_data)
      if (b.name == a.name) {
        b = std::move(a);
        return;
      }
    point_data.push_back(std::move(a));
  };
  const unsigned char none = 0;  // a valid pointer for an empty mesh
  add("MeanColoration", "UInt8", 3, 1, np ? (const void *)mean : &none);
  add("MedianColoration", "UInt8", 3, 1, np ? (const void *)median : &none);
  add("NbProjectedDepthMap", "Int32", 1, 4, np ? (const void *)count : &none);

  std::ofstream out(path, std::ios::binary);
  if (!out) {
    *error = "WriteColoredPolyData: cannot open " + path;
    return false;
  }
  // the XML first, every array appended in the order it is named; then the raw block: [UInt64 byte count] bytes, per array
  std::vector<const vtp::Array *> order;
  uint64_t offset = 0;
  std::ostringstream xml;
  auto array_tag = [&](const vtp::Array &a, const std::string &indent, const char *fallback_name) {
    xml << indent << "<DataArray type=\"" << a.type << "\" Name=\"" << (a.name.empty() ? fallback_name : a.name.c_str()) << "\"";
    if (a.components != 1) xml << " NumberOfComponents=\"" << a.components << "\"";
    xml << " format=\"appended\" offset=\"" << offset << "\"/>\n";
    offset += sizeof(uint64_t) + a.bytes.size();
    order.push_back(&a);
  };
  auto section = [&](const char *name, const std::vector<std::pair<std::string, std::string>> &designations,
                     const std::vector<vtp::Array> &arrays) {
    xml << "      <" << name;
    for (const auto &kv : designations) xml << " " << kv.first << "=\"" << kv.second << "\"";
    if (arrays.empty()) {
      xml << "/>\n";
      return;
    }
    xml << ">\n";
    for (const vtp::Array &a : arrays) array_tag(a, "        ", "");
    xml << "      </" << name << ">\n";
  };
  xml << "<?xml version=\"1.0\"?>\n<VTKFile type=\"PolyData\" version=\"1.0\" byte_order=\"LittleEndian\" header_type=\"UInt64\">\n"
         "  <PolyData>\n    <Piece NumberOfPoints=\""
      << mesh.n_points << "\" NumberOfVerts=\"0\" NumberOfLines=\"0\" NumberOfStrips=\"0\" NumberOfPolys=\"" << mesh.n_polys << "\">\n";
  section("PointData", mesh.point_designations, point_data);
  section("CellData", mesh.cell_designations, mesh.cell_data);
  xml << "      <Points>\n";
  array_tag(mesh.points, "        ", "Points");
  xml << "      </Points>\n      <Polys>\n";
  array_tag(mesh.connectivity, "        ", "connectivity");
  array_tag(mesh.offsets, "        ", "offsets");
  xml << "      </Polys>\n    </Piece>\n  </PolyData>\n  <AppendedData encoding=\"raw\">\n   _";
  const std::string head = xml.str();
  out.write(head.data(), (std::streamsize)head.size());
  for (const vtp::Array *a : order) {
    const uint64_t n = a->bytes.size();
    out.write(reinterpret_cast<const char *>(&n), sizeof(n));
    out.write(reinterpret_cast<const char *>(a->bytes.data()), (std::streamsize)n);
  }
  out << "\n  </AppendedData>\n</VTKFile>\n";
  if (!out) {
    *error = "WriteColoredPolyData: write failed: " + path;
    return false;
  }
  return true;
}

int Run(const Options &o, std::ostream &log, std::string *error) {
  auto say = [&](const std::string &what) {  // ShowInformation (cmain:140-146)
    if (o.verbose) log << what << "\n" << std::endl;
  };
  say("** Read input...");
  vtp::PolyData mesh;
  if (!vtp::ReadPolyData(o.input, &mesh, error)) return 1;
  // MeshColoration takes the points as f64 (vtkPoints::GetPoint); a Float32 file's values widen exactly
  const size_t np = (size_t)mesh.n_points;
  std::vector<double> points(np * 3);
  if (mesh.points.type == "Float64") {
    if (np) std::memcpy(points.data(), mesh.points.bytes.data(), np * 3 * sizeof(double));
  } else {
    for (size_t i = 0; i < np * 3; ++i) {
      float f;
      std::memcpy(&f, mesh.points.bytes.data() + 4 * i, 4);
      points[i] = (double)f;
    }
  }
  // --depthFromMesh: the polys as triangles, for the rendering only (the written polys are the input's); the views' files are then
  // read for their Color arrays alone and need no Depths
  std::vector<int64_t> triangles;
  if (o.depthFromMesh) {
    std::vector<int64_t> connectivity((size_t)(mesh.n_polys ? mesh.OffsetAt(mesh.n_polys - 1) : 0)), offsets((size_t)mesh.n_polys);
    for (size_t i = 0; i < connectivity.size(); ++i) connectivity[i] = mesh.ConnectivityAt((int64_t)i);
    for (size_t i = 0; i < offsets.size(); ++i) offsets[i] = mesh.OffsetAt((int64_t)i);
    triangles = FanTriangulate(connectivity.data(), (int64_t)connectivity.size(), offsets.data(), mesh.n_polys);
    say("** Depth of the visibility test: the input mesh, rendered (" + std::to_string(triangles.size() / 3) + " triangles)");
  }
  std::unique_ptr<MeshColoration> owner(o.depthFromMesh
                                            ? new MeshColoration(points.data(), (int64_t)np, triangles.data(), (int64_t)triangles.size() / 3, o.vti, o.krtd)
                                            : new MeshColoration(points.data(), (int64_t)np, o.vti, o.krtd));  // cmain:79
  MeshColoration &coloration = *owner;
  coloration.SetDevice(o.device);
  if (o.depthTest) coloration.SetDepthTolerance(o.depthTolerance);
  if (!coloration.ProcessColoration()) {  // cmain:80, 96-99
    say("Error during coloration process...");
    *error = coloration.LastError().empty() ? std::string("the coloration failed") : coloration.LastError();
    return 1;
  }
  say("** Write output image");  // cmain:84
  std::vector<int32_t> count(coloration.GetNbProjectedDepthMap().begin(), coloration.GetNbProjectedDepthMap().end());
  if (!WriteColoredPolyData(o.output, mesh, coloration.GetMeanColoration().data(), coloration.GetMedianColoration().data(),
                            count.data(), error))
    return 1;
  return 0;
}

}  // namespace color_cli
}  // namespace host
}  // namespace dmi
