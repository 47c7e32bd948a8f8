// k_catalog_nested<ISO_KIND_ISO, 1, 7 .. 12>
#include "nested_launch.h"

namespace iso {
namespace nestk {
ISO_DEFINE_NESTED_LAUNCHER(launch_nested_iso1_hi, ISO_KIND_ISO, 1, 7)
}  // namespace nestk
}  // namespace iso
