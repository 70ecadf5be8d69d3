// rt3_scene.hpp — what rt3_device.hip (the renders and queries) calls in rt3_scene.hip (the scene on the context).  The two units share state through
// struct rt3_ctx alone; these are the three places where the render unit needs the scene unit to act or to judge.  Inside the library
// only: hidden from its exports.
#pragma once
#include "rt3_ctx.hpp"

// A scene the trace kernels can take: every render and query asks first.  Lives with the scene because the scene unit's own rt3_debug_light_table asks too.
__attribute__((visibility("hidden"))) int check_scene(rt3_ctx* ctx);
// The sampling tables a call's flags need, built on `stream` by the first call that carries the flag (plan_sampled_trace): the builds launch the table
// kernels and the prefix sums, which belong to the scene unit as the tables' invalidation does.
__attribute__((visibility("hidden"))) int ensure_env_table(rt3_ctx* ctx, hipStream_t stream);
__attribute__((visibility("hidden"))) int ensure_light_table(rt3_ctx* ctx, hipStream_t stream);
