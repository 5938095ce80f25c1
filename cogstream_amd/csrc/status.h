// cogs_status values of include/cogs.h for the files that do not include it (the kernel files through common.h, attn_plan.h)
#pragma once
#define COGS_OK 0
#define COGS_E_INVALID (-1)
#define COGS_E_HIP (-2)
#define COGS_E_UNSUPPORTED (-3)
#define COGS_E_WORKSPACE (-4)
