// nms_tail_boxes.hip -- launch_tail for the from-boxes layer: the five tail_kernel<E, kFromBoxes> and nothing else (nms_layer.h)
#include "nms_tail_launch.h"

template int gnms_internal_launch_tail<gnms::kFromBoxes>(const gnms::LayerCall&, const float*, int64_t, int, int);
