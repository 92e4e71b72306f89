// bioinfo1_amd/csrc/ta_pipeline_internal.h -- what csrc/ta_pipeline.cpp uses of
// the library beyond include/team_align_c.h.  Included by ta_pipeline.cpp and
// by ta_api.hip (which defines it), so that the two cannot drift; not part of
// the public ABI.  ta_pipeline.cpp sees ta_context only as an opaque type (it
// is also built against a stand-in context by tests/cpp/pipeline_order.cpp).
#pragma once

#include "../../include/team_align_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sets the message ta_last_error(ctx) returns (null message: the empty string). */
void ta_context_set_error(ta_context* ctx, const char* message);

/* The traceback in two executions (team_align_c.h).  ta_pipeline.cpp refers to
 * them weakly (it defines TA_PIPELINE_WEAK_REFS): built against stand-ins that
 * define only the fill and the combined traceback (tests/cpp/pipeline_order.cpp,
 * pipeline_walk_streams.cpp) the references are null and every step takes the
 * combined call.  ta_api.hip, which defines them, sees the same declarations. */
#ifdef TA_PIPELINE_WEAK_REFS
#define TA_PIPELINE_REF __attribute__((weak))
#else
#define TA_PIPELINE_REF
#endif
TA_PIPELINE_REF int ta_plan_execute_walk(ta_plan* plan, const ta_device_io* io, void* hip_stream, uint32_t chunk);
TA_PIPELINE_REF int ta_plan_execute_format(ta_plan* plan, const ta_device_io* io, void* hip_stream, uint32_t chunk);
TA_PIPELINE_REF int ta_plan_format_is_split(const ta_plan* plan, uint32_t chunk);

#ifdef __cplusplus
}
#endif
