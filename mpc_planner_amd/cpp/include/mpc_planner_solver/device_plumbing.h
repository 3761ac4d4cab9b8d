/* mpc_planner_solver/device_plumbing.h -- what the batched twins (mpc_planner/data_preparation_batch.h, mpc_planner_modules/reference_path_batch.h, mpc_planner_modules/free_space_batch.h, mpc_planner_modules/guidance_handoff_batch.h, mpc_planner_modules/scenario_rows_batch.h)
 * share: device allocation, host-to-device copies on the handle's stream, the scene_of upload.  A failure prints "<class name>: <what>" on
 * stderr and exits.  Needs the HIP runtime header (compile with -D__HIP_PLATFORM_AMD__ and the ROCm include directory). */
#ifndef MPC_DEVICE_PLUMBING_HIP_H
#define MPC_DEVICE_PLUMBING_HIP_H

#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "tmpc_hip.h"

namespace MPCPlanner
{
    class DevicePlumbing
    {
    protected:
        DevicePlumbing(tmpc_handle *handle, const char *who) : _h(handle), _who(who) {}
        ~DevicePlumbing() { if (_d_scene_of) (void)hipFree(_d_scene_of); }
        void fail(const char *what) const { std::fprintf(stderr, "%s: %s\n", _who, what); std::exit(1); }
        void alloc(void *&p, size_t bytes) const { if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) fail("hipMalloc"); }
        void *stream() const { void *s = nullptr; if (tmpc_get_stream(_h, &s)) fail(tmpc_last_error(_h)); return s; }
        void copy(void *dst, const void *src, size_t bytes, void *stream) const
        {
            if (bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) fail("hipMemcpyAsync");
        }
        /* waits for the uploads enqueued so far: the host memory they read may end after this call */
        void sync(void *stream) const { if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) fail("hipStreamSynchronize"); }
        /* scene_of on the device, in a buffer that grows with the batch; synchronised: the caller's vector may end with the call */
        const void *uploadSceneOf(const std::vector<int> &scene_of)
        {
            void *s = stream();
            if (scene_of.size() > _n_scene_of) {
                if (_d_scene_of) (void)hipFree(_d_scene_of);
                alloc(_d_scene_of, scene_of.size() * sizeof(int)); _n_scene_of = scene_of.size();
            }
            copy(_d_scene_of, scene_of.data(), scene_of.size() * sizeof(int), s);
            sync(s);
            return _d_scene_of;
        }
        tmpc_handle *_h;
    private:
        const char *_who;
        void *_d_scene_of{nullptr};
        size_t _n_scene_of{0};
    };
}
#endif
