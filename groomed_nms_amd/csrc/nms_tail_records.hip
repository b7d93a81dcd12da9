// nms_tail_records.hip -- launch_tail for the from-records (3D) layer: the five tail_kernel<E, kFromRecords> and nothing else (nms_layer.h)
#include "nms_tail_launch.h"

template int gnms_internal_launch_tail<gnms::kFromRecords>(const gnms::LayerCall&, const float*, int64_t, int, int);
