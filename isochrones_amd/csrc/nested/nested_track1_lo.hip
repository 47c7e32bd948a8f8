// k_catalog_nested<ISO_KIND_TRACK, 1, 1 .. 6>
#include "nested_launch.h"

namespace iso {
namespace nestk {
ISO_DEFINE_NESTED_LAUNCHER(launch_nested_track1_lo, ISO_KIND_TRACK, 1, 1)
}  // namespace nestk
}  // namespace iso
