// TEST HELPERS: a generated unit compiled for the host, the preamble the *_emu.cpp programs of the march, profile, campaign,
// policy and sensitivity tests share.  RMT_HOST_EMULATION leaves out the kernels (their wave loops, lane indices and atomics
// are device-only); what the kernels call stays: the node function, the node solver rmt_steady_node, rmt_campaign_update and
// the per-node code of the sensitivity sweep.  RMT_GENERATED_SOURCE: the path of the unit's source (n2.plan_unit), quoted.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#define RMT_HOST_EMULATION 1
#define __device__
#define __forceinline__ inline
#define __restrict__
#ifndef INFINITY
#define INFINITY __builtin_inf()
#endif
using std::trunc;
#include RMT_GENERATED_SOURCE
