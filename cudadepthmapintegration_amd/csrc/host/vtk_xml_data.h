// vtk_xml_data.h -- the container decoding the VTK XML readers share (vti_reader.h: ImageData, vtp_reader.h: PolyData);
// defined in vti_reader.cpp.
//
// VTK is not in this image, so the format is restated from its published description (VTK file formats, "XML file
// formats"): <VTKFile type=... byte_order=... header_type="UInt32|UInt64" compressor="vtkZLibDataCompressor">; a
// <DataArray type=... Name=... NumberOfComponents=... format="ascii|binary|appended" offset=.../>; <AppendedData
// encoding="base64|raw"> _ DATA.  binary / appended payloads: [n_bytes] DATA, or with a compressor [n_blocks][block_size]
// [last_block_size][compressed size of each block] followed by the zlib-compressed blocks; header words are header_type;
// in base64 the header is its own base64 unit when compressed and shares the unit with the data when not.  LZ4 / LZMA
// compressors are refused (no codec in the image).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace dmi {
namespace host {
namespace vtkxml {

struct Array {
  std::string name;
  std::string type;   // "Float64", "UInt8", ... as written in the file
  int components = 1;
  size_t elem_size = 0;
  std::vector<unsigned char> bytes;  // host byte order, tuples * components * elem_size bytes
};

struct Format {
  size_t header_word = 4;  // header_type UInt32 (the default of version 0.1 files) or UInt64
  bool swap = false;       // file byte order differs from the host's
  bool zlib = false;
};

// Where the <AppendedData> payload starts (data == npos: the file has none) and how it is encoded.
struct Appended {
  size_t data = std::string::npos;
  bool raw = false;
};

bool Fail(std::string *err, const std::string &msg);  // *err = msg; false
// value of name="..." inside the text of one XML tag
bool Attr(const std::string &tag, const std::string &name, std::string *out);
// every name="value" pair of one tag, in order (the tag's own name excluded)
std::vector<std::pair<std::string, std::string>> Attributes(const std::string &tag);
size_t TypeSize(const std::string &type);  // 0: not a VTK numeric type
// byte_order / header_type / compressor of the <VTKFile> tag text
bool ReadFormat(const std::string &vtkfile_tag, const std::string &path, Format *fmt, std::string *err);
// the <AppendedData> section at or after `from`; *xml_end = where the XML that may be searched ends (raw payloads can contain
// anything: never search inside them)
bool FindAppended(const std::string &text, size_t from, const std::string &path, Appended *app, size_t *xml_end, std::string *err);
// Decodes the <DataArray> whose tag text is `tag` (ending at text[content - 1] = '>'): n_tuples tuples of the components
// and type the tag names (a->name / a->type / a->components / a->elem_size must be filled by the caller); inline content
// must end before `limit`.  *next = where the search for the next array goes on.  Host byte order on success.
bool DecodeDataArray(const std::string &text, const std::string &tag, bool self_closed, size_t content, size_t limit,
                     const Appended &app, const Format &fmt, size_t n_tuples, const std::string &path, Array *a, size_t *next,
                     std::string *err);

}  // namespace vtkxml
}  // namespace host
}  // namespace dmi
