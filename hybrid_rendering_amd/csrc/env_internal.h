// What env.hip (include/hr_env.h) and env_sources.hip (include/hr_env_sources.h) share: the hr_env object, the texel direction of hr_env.h's
// contract, and the second half of every update — the SH9 and prefilter launches over the env's own sky.
#pragma once
#include "hr_internal.h"
#include "shading.h"
#include "../../include/hr_env.h"

namespace hr {

// hr_env.h "Texel direction": the inverse of CubeMap::fetch, unnormalised
HR_DEV f3 texel_dir(int face, int x, int y, int s)
{
    const float u = 2.0f * __fdiv_rn((float)x + 0.5f, (float)s) - 1.0f;
    const float v = 2.0f * __fdiv_rn((float)y + 0.5f, (float)s) - 1.0f;
    switch (face)
    {
    case 0: return mk3(1.0f, -v, -u);
    case 1: return mk3(-1.0f, -v, u);
    case 2: return mk3(u, 1.0f, v);
    case 3: return mk3(u, -1.0f, -v);
    case 4: return mk3(u, -v, 1.0f);
    default: return mk3(-u, -v, -1.0f);
    }
}

} // namespace hr

struct hr_env
{
    hr_ctx*     ctx = nullptr;
    hr_env_desc d;
    size_t      chain_texels = 0;
    hr::DevBuf  sky, chain, lut, sh9, sh_rows, table, ht;
    hr::DevBuf  equirect_table;   // hr_env_sources.h contract 1: [6][S][S] (u, v); allocated and filled by the first hr_env_update_equirect
    hr::StageProfiler prof;
};

namespace hr {
// env.hip: the stages env_sh9 and env_prefilter over e->sky on `st` (the device is set, the profiler's frame is begun by the caller)
hr_status env_enqueue_derived(hr_env* e, hipStream_t st);
} // namespace hr
