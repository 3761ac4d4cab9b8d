/*
 * mpc_planner_modules/reference_path_batch.h -- the batched device twin of mpc_planner_modules/reference_path.h, next to
 * mpc_planner/data_preparation_batch.h: the whole paths of several scenes (and their bound cubics) are uploaded ONCE -- fitted cubics with
 * setPaths(), or raw waypoints with setWaypoints(), which tmpc_fit_path turns into the cubics on the device --; per tick track()
 * enqueues tmpc_track_path -- closest point from the previous segment, the window of S segments, the bound window, the objective-reached flag
 * -- and setParameters() enqueues tmpc_set_path_parameters, which writes the spline columns of the handle's current batch and, optionally,
 * the `spline` entry of a device state buffer: what Contouring::update / setSplineParameters do per scene on the host (contouring.cpp:28-48,
 * :94-124), bit for bit.  boundWindow() is then ready for tmpc_road_halfspaces (d_bound_segments).  With a velocity at every waypoint of
 * every path, setWaypoints() also fits the velocity profiles (PathReferenceVelocity::onDataReceived) and setVelocityParameters() enqueues
 * tmpc_path_velocity_window and tmpc_scatter_parameters: the spline_v columns of a generated stack, and referenceVelocity() for the guidance
 * planner (path_reference_velocity.cpp:59-95, guidance_constraints.cpp:91-94).  In a generated solver, whose handle has no S, track() passes the
 * twin's S as tmpc_path_options::window_segments; after setColumns() -- the 9 S spline columns of the stack's parameter map -- setParameters()
 * and roadHalfspaces() go through include/tmpc_hip_stack_env.h (tmpc_stack_set_path_columns, tmpc_stack_road_halfspaces), the same kernels with
 * the columns named by the caller; without setColumns() nothing changes.  For callers of the C-ABI
 * (include/tmpc_hip.h) that keep a launch of many scenes on the device; needs the HIP runtime header (compile with -D__HIP_PLATFORM_AMD__
 * and the ROCm include directory).  Everything is enqueued on the handle's stream; setPaths() and setParameters() wait for their own uploads
 * (the staging memory is their own), not for the kernels.
 */
#ifndef MPC_REFERENCE_PATH_BATCH_HIP_H
#define MPC_REFERENCE_PATH_BATCH_HIP_H

#include <mpc_planner_modules/reference_path.h>
#include <mpc_planner_solver/device_plumbing.h>

#include "tmpc_hip_stack_env.h"

namespace MPCPlanner
{
    class BatchedPathTracking : private DevicePlumbing
    {
    public:
        /* n_scenes paths of up to n_seg_max (<= 1024) segments each; S = the solver's window (tmpc_dims::S) */
        BatchedPathTracking(tmpc_handle *handle, int n_scenes, int n_seg_max, int S, bool with_bounds)
            : DevicePlumbing(handle, "BatchedPathTracking"), _Q(n_scenes), _R(n_seg_max), _S(S), _with_bounds(with_bounds)
        {
            const size_t Q = (size_t)_Q, R = (size_t)_R, W = (size_t)_S;
            alloc(_d_path, Q * R * 9 * 8); alloc(_d_count, Q * sizeof(int)); alloc(_d_length, Q * 8); alloc(_d_segment, Q * sizeof(int));
            alloc(_d_closest_s, Q * 8); alloc(_d_window, Q * W * 9 * 8); alloc(_d_reached, Q);
            if (_with_bounds) { alloc(_d_bounds, Q * 2 * R * 8 * 8); alloc(_d_bound_window, Q * 2 * W * 8 * 8); }
        }
        ~BatchedPathTracking()
        {
            for (void *p : {_d_path, _d_count, _d_length, _d_segment, _d_closest_s, _d_window, _d_reached, _d_bounds, _d_bound_window, _d_waypoints, _d_status, _d_road_width,
                            _d_velocity, _d_velocity_window, _d_v_ref}) if (p) (void)hipFree(p);
        }
        BatchedPathTracking(const BatchedPathTracking &) = delete;
        BatchedPathTracking &operator=(const BatchedPathTracking &) = delete;

        /* New paths for every scene (segments beyond n_seg_max are not seen; with_bounds: left_bound / right_bound one cubic per segment).
         * Like Contouring::onDataReceived("reference_path") (:126-157): every scene's previous segment goes back to -1, the next track()
         * searches every segment. */
        void setPaths(const std::vector<ReferencePathSpline> &paths)
        {
            const size_t Q = (size_t)_Q, R = (size_t)_R;
            if (paths.size() != Q) fail("setPaths: one path per scene");
            _with_velocity = false;                                           // fitted cubics carry no velocity profile
            std::vector<double> path(Q * R * 9, 0.), length(Q, 0.), bounds(_with_bounds ? Q * 2 * R * 8 : 0, 0.);
            std::vector<int> count(Q), segment(Q, -1);
            for (size_t q = 0; q < Q; q++) {
                const ReferencePathSpline &p = paths[q];
                count[q] = (int)(p.segments.size() < R ? p.segments.size() : R);
                length[q] = p.length;
                if (_with_bounds && (p.left_bound.size() < (size_t)count[q] || p.right_bound.size() < (size_t)count[q])) fail("setPaths: a bound cubic per segment");
                for (size_t i = 0; i < (size_t)count[q]; i++) {
                    coefficients(p.segments[i], &path[(q * R + i) * 9]); path[(q * R + i) * 9 + 8] = p.segments[i].start;
                    if (_with_bounds) { coefficients(p.left_bound[i], &bounds[((q * 2 + 0) * R + i) * 8]); coefficients(p.right_bound[i], &bounds[((q * 2 + 1) * R + i) * 8]); }
                }
            }
            void *stream = this->stream();
            copy(_d_path, path.data(), path.size() * 8, stream); copy(_d_count, count.data(), Q * sizeof(int), stream);
            copy(_d_length, length.data(), Q * 8, stream); copy(_d_segment, segment.data(), Q * sizeof(int), stream);
            if (_with_bounds) copy(_d_bounds, bounds.data(), bounds.size() * 8, stream);
            sync(stream);                                                     // the staging vectors end with this call
        }
        /* The alternative to setPaths(): raw waypoints for every scene, fitted ON THE DEVICE (tmpc_fit_path) into the twin's own
         * path / count / length / bound buffers -- bit for bit what ReferencePathSpline::fit / fitBounds give on the host.  One upload (the
         * waypoints of all scenes, their bounds, their s and the counts in one staging block), one kernel.  Waypoints beyond n_seg_max + 1
         * are not seen.  Knots: the paths' s if EVERY path carries one, chord lengths if none does.  with_bounds: left / right hold one
         * Boundary per scene with the centreline's point count.  An invalid scene (fewer than two waypoints, a repeated waypoint) gets
         * count 0: track() leaves it alone; status() tells.  Every scene's previous segment goes back to -1.  When EVERY path has a velocity
         * at each waypoint (ReferencePath::hasVelocity) the velocity profiles are fitted in the same launch, on the centreline's knots;
         * otherwise no scene has a profile and setVelocityParameters() writes the constant reference velocity. */
        void setWaypoints(const std::vector<ReferencePath> &paths, const std::vector<Boundary> *left = nullptr, const std::vector<Boundary> *right = nullptr)
        {
            const size_t Q = (size_t)_Q, P = (size_t)_R + 1;
            if (paths.size() != Q) fail("setWaypoints: one path per scene");
            if (_with_bounds && (!left || !right || left->size() != Q || right->size() != Q)) fail("setWaypoints: a left and a right bound per scene");
            size_t with_s = 0;
            for (const ReferencePath &p : paths) with_s += p.hasDistance() ? 1 : 0;
            if (with_s != 0 && with_s != Q) fail("setWaypoints: s for every path or for none");
            size_t with_v = 0;
            for (const ReferencePath &p : paths) with_v += p.hasVelocity() ? 1 : 0;
            _with_velocity = with_v == Q;
            // one staging block: xy [Q][P][2], s [Q][P], left [Q][P][2], right [Q][P][2], v [Q][P] (doubles), then count and segment [Q] each (ints)
            const size_t o_xy = 0, o_s = o_xy + Q * P * 2, o_left = o_s + Q * P, o_right = o_left + Q * P * 2, o_v = o_right + Q * P * 2, n_dbl = o_v + Q * P;
            const size_t bytes = n_dbl * 8 + 2 * Q * sizeof(int);
            std::vector<double> stage(n_dbl + (2 * Q * sizeof(int) + 7) / 8, 0.);
            int *count = reinterpret_cast<int *>(stage.data() + n_dbl), *segment = count + Q;
            for (size_t q = 0; q < Q; q++) {
                const ReferencePath &p = paths[q];
                if (p.y.size() != p.x.size() || (p.hasDistance() && p.s.size() != p.x.size())) fail("setWaypoints: x, y and s of one length");
                if (_with_velocity && p.v.size() != p.x.size()) fail("setWaypoints: a velocity per waypoint");
                const size_t n = p.x.size() < P ? p.x.size() : P;
                count[q] = (int)n; segment[q] = -1;
                if (_with_bounds)
                    for (const Boundary *b : {&(*left)[q], &(*right)[q]}) if (b->x.size() != p.x.size() || b->y.size() != p.x.size()) fail("setWaypoints: the bounds need the centreline's point count");
                for (size_t i = 0; i < n; i++) {
                    stage[o_xy + (q * P + i) * 2] = p.x[i]; stage[o_xy + (q * P + i) * 2 + 1] = p.y[i];
                    if (with_s) stage[o_s + q * P + i] = p.s[i];
                    if (_with_velocity) stage[o_v + q * P + i] = p.v[i];
                    if (_with_bounds) {
                        stage[o_left + (q * P + i) * 2] = (*left)[q].x[i]; stage[o_left + (q * P + i) * 2 + 1] = (*left)[q].y[i];
                        stage[o_right + (q * P + i) * 2] = (*right)[q].x[i]; stage[o_right + (q * P + i) * 2 + 1] = (*right)[q].y[i];
                    }
                }
            }
            if (!_d_waypoints) { alloc(_d_waypoints, bytes); alloc(_d_status, Q); alloc(_d_road_width, Q * 8); }
            if (_with_velocity && !_d_velocity) alloc(_d_velocity, Q * (size_t)_R * 4 * 8);
            void *stream = this->stream();
            copy(_d_waypoints, stage.data(), bytes, stream);
            double *base = static_cast<double *>(_d_waypoints);
            int *d_count_in = reinterpret_cast<int *>(base + n_dbl);
            if (hipMemcpyAsync(_d_segment, d_count_in + Q, Q * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) fail("hipMemcpyAsync");
            if (tmpc_fit_path(_h, _Q, (int)P, _R, base + o_xy, d_count_in, with_s ? base + o_s : nullptr, _with_bounds ? base + o_left : nullptr,
                              _with_bounds ? base + o_right : nullptr, _with_velocity ? base + o_v : nullptr, _d_path, _d_count, _d_length,
                              _with_bounds ? _d_bounds : nullptr, _with_velocity ? _d_velocity : nullptr,
                              _with_bounds ? _d_road_width : nullptr, _d_status)) fail(tmpc_last_error(_h));
            sync(stream);                                                     // the staging vector ends with this call
        }
        /* after setWaypoints(): per scene 0 = fitted, 1 = invalid (u8), and with bounds the road width (f64); device buffers */
        const void *status() const { return _d_status; }
        const void *roadWidth() const { return _d_road_width; }
        /* the fitted (or uploaded) whole paths: [n_scenes][n_seg_max][9], i32 [n_scenes], f64 [n_scenes], [n_scenes][2][n_seg_max][8] or nullptr */
        const void *paths() const { return _d_path; }
        const void *pathCounts() const { return _d_count; }
        const void *pathLengths() const { return _d_length; }
        const void *bounds() const { return _d_bounds; }

        /* Contouring::reset() for every scene: the next track() searches every segment */
        void reset()
        {
            const std::vector<int> segment((size_t)_Q, -1);
            void *stream = this->stream();
            copy(_d_segment, segment.data(), segment.size() * sizeof(int), stream);
            sync(stream);
        }

        /* One tick of Contouring::update for every scene: d_pos f64 [n_scenes][pos_stride] on the device, x and y first (a state buffer as
         * tmpc_prepare_obstacles or tmpc_warmstart read it can be passed as it is).  Enqueued; nothing is read back. */
        void track(const void *d_pos, int pos_stride, int search_range = 2)
        {
            tmpc_path_options opt{};
            opt.size = sizeof(opt); opt.search_range = search_range; opt.window_segments = _S;     /* a generated solver's handle has no S of its own */
            if (tmpc_track_path(_h, _Q, _R, _d_path, _d_count, _d_length, _d_bounds, d_pos, pos_stride, &opt, _d_segment, _d_closest_s, _d_window, _d_bound_window,
                                _d_reached)) fail(tmpc_last_error(_h));
        }

        /* Column mode, for a handle of a GENERATED library: path_cols = the 9 S columns of the stack's parameter map (parameter_map.yaml) in the
         * window's order, spline_x{i}_a .. _d, spline_y{i}_a .. _d, spline{i}_start for i = 0 .. S - 1.  From then on setParameters() and
         * roadHalfspaces() use tmpc_stack_set_path_columns and tmpc_stack_road_halfspaces. */
        void setColumns(const std::vector<int32_t> &path_cols)
        {
            if ((int)path_cols.size() != 9 * _S) fail("setColumns: 9 S columns");
            _columns = true; _path_cols = path_cols;
        }

        /* The spline columns of the handle's CURRENT batch (tmpc_set_batch* first): scene_of[b] = scene of batch entry b, outside [0, n_scenes):
         * the entry is left alone.  d_state != nullptr (device, [B][nx], the layout tmpc_warmstart reads): its `spline` entry becomes the
         * scene's closest_s -- before tmpc_warmstart(d_state) the solve starts from the fresh value, after it from the previous tick's, as in
         * the reference (planner.cpp:81-96).  Column mode: into path_cols (tmpc_stack_set_path_columns); otherwise tmpc_set_path_parameters. */
        void setParameters(const std::vector<int> &scene_of, void *d_state = nullptr)
        {
            const void *d_scene_of = uploadSceneOf(scene_of);
            const int rc = _columns ? tmpc_stack_set_path_columns(_h, _path_cols.data(), _S, _d_window, d_scene_of, _Q, d_state ? _d_closest_s : nullptr, d_state)
                                    : tmpc_set_path_parameters(_h, _d_window, d_scene_of, _Q, d_state ? _d_closest_s : nullptr, d_state);
            if (rc) fail(tmpc_last_error(_h));
        }

        /* Contouring's road rows (contouring.cpp:181-262) for every scene, after setParameters(): rows first_row, first_row + 1 of
         * d_static_halfspaces f64 [n_scenes][N][n_static][3] (device; what tmpc_linearize_topology_ex / tmpc_stack_linearize_topology_columns read)
         * from the warm start and the path window of batch entry d_main_of[q] (i32 [n_scenes], device).  from_bounds: bounds mode on
         * boundWindow() (the twin was built with_bounds), offset_first = offset_second = the robot radius; otherwise centreline mode.  Column
         * mode: tmpc_stack_road_halfspaces; otherwise tmpc_road_halfspaces.  Enqueued. */
        void roadHalfspaces(const void *d_main_of, double offset_first, double offset_second, void *d_static_halfspaces, int n_static, int first_row = 0,
                            bool from_bounds = false)
        {
            if (from_bounds && !_with_bounds) fail("roadHalfspaces: from_bounds needs a twin with bounds");
            const void *bounds = from_bounds ? _d_bound_window : nullptr;
            const int rc = _columns ? tmpc_stack_road_halfspaces(_h, _path_cols.data(), _S, d_main_of, _Q, bounds, offset_first, offset_second, d_static_halfspaces, n_static, first_row)
                                    : tmpc_road_halfspaces(_h, d_main_of, _Q, bounds, offset_first, offset_second, d_static_halfspaces, n_static, first_row);
            if (rc) fail(tmpc_last_error(_h));
        }

        /* The same columns in a GENERATED solver, where tmpc_set_path_parameters refuses: cols = the 9 S columns of the stack's parameter map in
         * the window's order, spline_x{i}_a .. _d, spline_y{i}_a .. _d, spline{i}_start for i = 0 .. S - 1 (tmpc_scatter_parameters). */
        void setSplineParameters(const std::vector<int> &scene_of, const std::vector<int32_t> &cols)
        {
            if ((int)cols.size() != 9 * _S) fail("setSplineParameters: 9 S columns");
            if (tmpc_scatter_parameters(_h, cols.data(), (int32_t)cols.size(), _d_window, 0, uploadSceneOf(scene_of), _Q)) fail(tmpc_last_error(_h));
        }
        /* PathReferenceVelocity::setParameters for every scene, after track(): the S velocity cubics from the segment found on -- zeros beyond
         * the path's end, (0, 0, 0, reference_velocity) without profiles -- into cols, the 4 S columns spline_v{i}_a .. _d, i = 0 .. S - 1, of every
         * stage of every entry of the CURRENT batch whose scene_of is inside [0, n_scenes); and referenceVelocity().  Enqueued. */
        void setVelocityParameters(const std::vector<int> &scene_of, const std::vector<int32_t> &cols, double reference_velocity)
        {
            if ((int)cols.size() != 4 * _S) fail("setVelocityParameters: 4 S columns");
            if (!_d_velocity_window) { alloc(_d_velocity_window, (size_t)_Q * _S * 4 * 8); alloc(_d_v_ref, (size_t)_Q * 8); }
            if (tmpc_path_velocity_window(_h, _Q, _R, _S, _with_velocity ? _d_velocity : nullptr, _d_path, _d_count, _d_length, _d_segment, _d_closest_s, nullptr,
                                          reference_velocity, _d_velocity_window, _d_v_ref)) fail(tmpc_last_error(_h));
            if (tmpc_scatter_parameters(_h, cols.data(), (int32_t)cols.size(), _d_velocity_window, 0, uploadSceneOf(scene_of), _Q)) fail(tmpc_last_error(_h));
        }
        /* after setVelocityParameters(): f64 [n_scenes], the profile at closest_s (or reference_velocity): what the guidance planner is given
         * (guidance_constraints.cpp:91-94); the window [n_scenes][S][4]; the fitted profiles [n_scenes][n_seg_max][4] or nullptr.  Device buffers */
        const void *referenceVelocity() const { return _d_v_ref; }
        const void *velocityWindow() const { return _d_velocity_window; }
        const void *velocities() const { return _with_velocity ? _d_velocity : nullptr; }

        /* device buffers, valid after track(): the window [n_scenes][S][9], the bound window [n_scenes][2][S][8] (what tmpc_road_halfspaces takes
         * as d_bound_segments; nullptr without bounds), closest_s [n_scenes], the segment found (i32) and the reached flag (u8) per scene */
        const void *window() const { return _d_window; }
        const void *boundWindow() const { return _d_bound_window; }
        const void *closestS() const { return _d_closest_s; }
        const void *segments() const { return _d_segment; }
        const void *reached() const { return _d_reached; }
        /* ModuleData::current_path_segment and closest_s of every scene; synchronises the handle's stream */
        void current(std::vector<int> &segment, std::vector<double> &closest_s) const
        {
            segment.assign((size_t)_Q, -1); closest_s.assign((size_t)_Q, 0.);
            if (tmpc_synchronize(_h)) fail(tmpc_last_error(_h));
            if (hipMemcpy(segment.data(), _d_segment, segment.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) fail("hipMemcpy");
            if (hipMemcpy(closest_s.data(), _d_closest_s, closest_s.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) fail("hipMemcpy");
        }

    private:
        int _Q, _R, _S;
        bool _with_bounds, _with_velocity{false};
        bool _columns{false};
        std::vector<int32_t> _path_cols;
        void *_d_path{nullptr}, *_d_count{nullptr}, *_d_length{nullptr}, *_d_segment{nullptr}, *_d_closest_s{nullptr}, *_d_window{nullptr}, *_d_reached{nullptr};
        void *_d_bounds{nullptr}, *_d_bound_window{nullptr};
        void *_d_waypoints{nullptr}, *_d_status{nullptr}, *_d_road_width{nullptr};       /* setWaypoints(): allocated on its first call */
        void *_d_velocity{nullptr}, *_d_velocity_window{nullptr}, *_d_v_ref{nullptr};    /* the velocity profiles: allocated on first use */
    };
}
#endif
