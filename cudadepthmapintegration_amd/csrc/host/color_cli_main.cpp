// dmi_coloration -- the reference's `Coloration` command line (Coloration/main.cxx:69-101) over libdmi_hip.so.
#include "../../../include/dmi_host.h"

int main(int argc, char **argv) { return dmi_color_cli_main(argc, argv); }
