// nms_tail_write_records.hip -- launch_tail_write for the 3D one-call entry: the ten tail_write_kernel<VEC, E, kFromRecords> and nothing
// else (nms_layer.h)
#include "nms_tail_write_launch.h"

template int gnms_internal_launch_tail_write<gnms::kFromRecords>(const gnms::LayerCall&, const float*, const float*, float*, int64_t);
