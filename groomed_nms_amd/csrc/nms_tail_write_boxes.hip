// nms_tail_write_boxes.hip -- launch_tail_write for the 2D one-call entry: the ten tail_write_kernel<VEC, E, kFromBoxes> and nothing else
// (nms_layer.h)
#include "nms_tail_write_launch.h"

template int gnms_internal_launch_tail_write<gnms::kFromBoxes>(const gnms::LayerCall&, const float*, const float*, float*, int64_t);
