// gtop_capi_time.h — what the entry points of include/gtop_time.h (gtop_capi_time.cpp) and of
// include/gtop_time_moving.h (gtop_capi_time_moving.cpp) share: the rules of a call and the cost's parameters.
#ifndef GTOP_CAPI_TIME_H_
#define GTOP_CAPI_TIME_H_

#include "gtop_ctx.h"
#include "gtop_time.h"

// what every device form asks of the context and of a call of B rows of m segments, before anything is launched;
// refuse_moving: GTOP_ERR_STATE while gtop_set_moving_cost is switched on (gtop_time.h's rule)
int gtop_time_ready(gtop_ctx *c, const char *who, int B, int m, int time_stride, bool refuse_moving);
// the rules of gtop_timeopt
int gtop_check_timeopt(gtop_ctx *c, const gtop_timeopt *o);
// the context's gtop_params as the time kernels take them
GtopTimeCost gtop_time_cost(const gtop_ctx *c);

#endif  // GTOP_CAPI_TIME_H_
