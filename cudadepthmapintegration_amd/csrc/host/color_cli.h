// color_cli.h -- the command line of the reference's `Coloration` tool (Coloration/main.cxx, "cmain") on top of the host
// mirror: the same flags and checks (cmain:105-135), the mesh read from a .vtp (vtkXMLPolyDataReader, cmain:75-77: here
// vtp_reader.h), MeshColoration over the two list files (cmain:79-80), and the mesh written back with its three new point
// arrays (vtkXMLPolyDataWriter, cmain:85-88).  Not in the reference: --device, --depthTolerance, which turns on the
// visibility test of dmi_color_set_depth_test, and --depthFromMesh, which gives that test the input mesh's own rendered depth
// (dmi_color_render_depths) instead of the views' "Depths" arrays.  One deliberate deviation: when the colouring fails the reference still returns
// EXIT_SUCCESS, writes nothing and says so only under --verbose (cmain:82-99); this tool returns 1 and prints the error.
#pragma once

#include <cstdint>
#include <iosfwd>
#include <string>

#include "vtp_reader.h"

namespace dmi {
namespace host {
namespace color_cli {

struct Options {
  std::string input;   // --input (.vtp, required)
  std::string output;  // --output (.vtp, required)
  std::string krtd;    // --krtd: the list file of .krtd paths (required)
  std::string vti;     // --vti: the list file of .vti paths (required)
  bool verbose = false;
  int device = 0;                // --device (not in the reference)
  bool depthTest = false;        // --depthTolerance given (not in the reference)
  double depthTolerance = 0.0;
  bool depthFromMesh = false;    // --depthFromMesh: the test's depth is the input mesh's own, rendered (not in the reference)
};

// cmain:105-135.  false: do not run (an error or --help; the text went to `err`).
bool ReadArguments(int argc, const char *const *argv, Options *out, std::ostream &err);
std::string HelpText();
// cmain:69-101.  0 on success; 1 with *error when the mesh cannot be read, coloured or written.  `log` receives what --verbose
// prints.
int Run(const Options &o, std::ostream &log, std::string *error);

// The mesh as MeshColoration leaves it (MC.cxx:55 DeepCopy, :194-196 AddArray): points in their input type, the polys, every
// input point- and cell-data array with its designations, and the point arrays MeanColoration (UInt8 x 3), MedianColoration
// (UInt8 x 3) and NbProjectedDepthMap (Int32) -- an input array of one of these names is replaced in place, as
// vtkFieldData::AddArray does.  VTK XML PolyData, appended raw data, UInt64 headers, little-endian (the layout of
// cli::WritePolyData).
bool WriteColoredPolyData(const std::string &path, const vtp::PolyData &mesh, const uint8_t *mean, const uint8_t *median,
                          const int32_t *count, std::string *error);

}  // namespace color_cli
}  // namespace host
}  // namespace dmi
