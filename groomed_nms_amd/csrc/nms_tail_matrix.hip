// nms_tail_matrix.hip -- launch_tail for the layer from the matrix: the five tail_kernel<E, kFromMatrix> and nothing else (nms_layer.h)
#include "nms_tail_launch.h"

template int gnms_internal_launch_tail<gnms::kFromMatrix>(const gnms::LayerCall&, const float*, int64_t, int, int);
