// The reference path in C++ (mpc_planner_modules/reference_path.h: closest point, segment window, objective reached -- DESIGN.md U14).
// Two programs from this file, both driven by tests/test_cpp_path.py:
//   (default)            Solver-free, g++ only, CPU:  test_reference_path <scenes.bin>
//       scenes.bin: n_scenes n_seg_max S search_range with_bounds; per scene: count length previous_segment px py, n_seg_max x 9 path numbers,
//       2 x n_seg_max x 8 bound numbers (present in either mode).  Prints per scene with count > 0 (count clipped to n_seg_max):
//       "scene q segment s reached", "w q slot 9 numbers", with bounds "l q slot 8 numbers" and "r q slot 8 numbers" -- %.17g round-trips a double.
//   -DWITH_SOLVER         Contouring::update in path mode on a generated solver (needs a GPU: the Solver owns a device handle):
//       test_reference_path_solver <config dir> <scene.bin>
//       scene.bin: N S; 8 weights; robot radius; state (x y psi v spline); n_path, n_path x 9, length; n_ticks, per tick (x y new_path).
//       Prints per tick "tick t current_path_segment spline reached" and the parameter rows of stages 0 and N - 1 ("p t k ...");
//       then the batched device twin (reference_path_batch.h) against ReferencePathSpline on the host: "batch differ 0 ...".
#ifdef WITH_SOLVER
#include <mpc_planner_modules/modules_hip.h>
#include <mpc_planner_modules/reference_path_batch.h>
#include <algorithm>
#include <cstring>
#else
#include <mpc_planner_modules/reference_path.h>
#endif

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace MPCPlanner;

static std::vector<double> read_all(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); std::exit(2); }
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    std::vector<double> v(n / 8);
    if (std::fread(v.data(), 8, v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
    return v;
}

#ifndef WITH_SOLVER
struct Point { double v[2]; double operator()(int i) const { return v[i]; } };

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::vector<double> in = read_all(argv[1]);
    size_t o = 0;
    auto next = [&]() { return in.at(o++); };
    const int n_scenes = (int)next(), n_seg_max = (int)next(), S = (int)next(), range = (int)next(), with_bounds = (int)next();
    for (int q = 0; q < n_scenes; q++) {
        int count = (int)next();
        const double length = next();
        int segment = (int)next();
        const Point p{{in.at(o), in.at(o + 1)}}; o += 2;
        const size_t path_at = o, bounds_at = o + (size_t)n_seg_max * 9;
        o = bounds_at + (size_t)2 * n_seg_max * 8;
        count = count > n_seg_max ? n_seg_max : count;
        if (count <= 0) continue;
        ReferencePathSpline path;
        path.length = length;
        auto seg_at = [&](size_t at, bool with_start) {
            PathSegment s{in[at], in[at + 1], in[at + 2], in[at + 3], in[at + 4], in[at + 5], in[at + 6], in[at + 7], with_start ? in[at + 8] : 0.};
            return s;
        };
        for (int i = 0; i < count; i++) {
            path.segments.push_back(seg_at(path_at + (size_t)i * 9, true));
            if (with_bounds) {
                path.left_bound.push_back(seg_at(bounds_at + (size_t)i * 8, false));
                path.right_bound.push_back(seg_at(bounds_at + ((size_t)n_seg_max + i) * 8, false));
            }
        }
        double s = 0.;
        path.findClosestPoint(p, segment, s, range);
        std::printf("scene %d %d %.17g %d\n", q, segment, s, (int)path.reached(p));
        std::vector<PathSegment> win, left, right;
        path.window(segment, S, win, &left, &right);
        for (int w = 0; w < S; w++) {
            const PathSegment &c = win[w];
            std::printf("w %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", q, w, c.ax, c.bx, c.cx, c.dx, c.ay, c.by, c.cy, c.dy, c.start);
        }
        if (with_bounds)
            for (int side = 0; side < 2; side++)
                for (int w = 0; w < S; w++) {
                    const PathSegment &c = side ? right[w] : left[w];
                    std::printf("%c %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", side ? 'r' : 'l', q, w, c.ax, c.bx, c.cx, c.dx, c.ay, c.by, c.cy, c.dy);
                }
    }
    return 0;
}
#else
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    setSolverConfigPath(argv[1]);
    const std::vector<double> in = read_all(argv[2]);
    size_t o = 0;
    auto next = [&]() { return in.at(o++); };
    const int N = (int)next(), S = (int)next();
    if (N != SOLVER_N || S != SOLVER_S) { std::printf("scene does not match the generated solver\n"); return 2; }
    ModuleConfig cfg;
    cfg.num_segments = S;
    const char *wn[] = {"acceleration", "angular_velocity", "velocity", "reference_velocity", "contour", "lag", "terminal_angle", "terminal_contouring"};
    for (int i = 0; i < 8; i++) cfg.weights[wn[i]] = next();
    cfg.robot_radius = next();
    State state;
    const char *sn[] = {"x", "y", "psi", "v", "spline"};
    for (int i = 0; i < 5; i++) state.set(sn[i], next());
    RealTimeData data;
    data.robot_area.emplace_back(0., cfg.robot_radius);
    const int n_path = (int)next();
    for (int i = 0; i < n_path; i++) {
        PathSegment sg;
        sg.ax = next(); sg.bx = next(); sg.cx = next(); sg.dx = next(); sg.ay = next(); sg.by = next(); sg.cy = next(); sg.dy = next(); sg.start = next();
        data.reference_path.push_back(sg);
    }
    data.reference_path_length = next();
    auto solver = std::make_shared<Solver>(0);
    MPCBaseModule base(solver, cfg, {"acceleration", "angular_velocity", "velocity", "reference_velocity"});
    Contouring contouring(solver, cfg);
    ModuleData module_data;
    const int n_ticks = (int)next();
    for (int t = 0; t < n_ticks; t++) {
        const double x = next(), y = next();
        const bool new_path = next() != 0.;
        state.set("x", x); state.set("y", y);
        if (new_path) contouring.onDataReceived(data, "reference_path");
        contouring.update(state, data, module_data);
        std::printf("tick %d %d %.17g %d %zu\n", t, module_data.current_path_segment, state.get("spline"), (int)contouring.isObjectiveReached(state, data),
                    module_data.path.size());
        for (int k = 0; k < N; k++) { base.setParameters(data, module_data, k); contouring.setParameters(data, module_data, k); }
        for (int k : {0, N - 1}) {
            std::printf("p %d %d", t, k);
            for (int i = 0; i < SOLVER_NP; i++) std::printf(" %.17g", solver->_params.all_parameters[k * SOLVER_NP + i]);
            std::printf("\n");
        }
    }
    contouring.reset();
    contouring.update(state, data, module_data);
    std::printf("reset %d\n", module_data.current_path_segment);

    // ---- the batched device twin (mpc_planner_modules/reference_path_batch.h): two scenes -- the whole path with bounds, and its first three
    // segments (fewer than S: padded slots) --, six batch entries of which entry 2 names no scene; against ReferencePathSpline on the host, bitwise
    const int Q = 2, B = 6;
    std::vector<ReferencePathSpline> paths(Q);
    for (int q = 0; q < Q; q++) {
        const size_t n = q == 0 ? data.reference_path.size() : 3;
        paths[q].segments.assign(data.reference_path.begin(), data.reference_path.begin() + n);
        paths[q].length = q == 0 ? data.reference_path_length : data.reference_path[3].start;
        for (size_t i = 0; i < n; i++) {
            PathSegment l = data.reference_path[i], r = data.reference_path[i];
            l.dy += 2.0; r.dy -= 1.5; r.by += 0.01;
            paths[q].left_bound.push_back(l); paths[q].right_bound.push_back(r);
        }
    }
    const double pos[Q][4] = {{9.3, 0.4, 0., 1.}, {7.7, -0.2, 0., 1.}};
    const std::vector<int> scene_of = {0, 0, -1, 1, 1, 1};
    tmpc_dims d;
    tmpc_default_dims_ex(&d, SOLVER_N, SOLVER_S, SOLVER_NLIN, SOLVER_M, SOLVER_NSLK, SOLVER_SLACK);
    tmpc_handle *h = nullptr;
    if (tmpc_create(&h, &d, B, 0)) { std::printf("tmpc_create failed\n"); return 1; }
    std::vector<double> xinit((size_t)B * SOLVER_NX, 0.), x0((size_t)B * (N + 1) * (SOLVER_NX + SOLVER_NU), 0.), start((size_t)B * N * SOLVER_NP, -7.);
    if (tmpc_set_batch(h, B, xinit.data(), x0.data(), start.data())) { std::printf("%s\n", tmpc_last_error(h)); return 1; }
    void *d_pos = nullptr, *d_state = nullptr;
    std::vector<double> st((size_t)B * SOLVER_NX, 9.);
    if (hipMalloc(&d_pos, sizeof(pos)) != hipSuccess || hipMalloc(&d_state, st.size() * 8) != hipSuccess) return 1;
    if (hipMemcpy(d_pos, pos, sizeof(pos), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_state, st.data(), st.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return 1;
    {
        BatchedPathTracking twin(h, Q, (int)data.reference_path.size(), S, true);
        twin.setPaths(paths);
        size_t differ = 0, written = 0, state_differ = 0, bound_differ = 0;
        int segment_differ = 0;
        for (int tick = 0; tick < 2; tick++) {                                   // a global search, then a local one from the segment found
            twin.track(d_pos, 4);
            twin.setParameters(scene_of, d_state);
            std::vector<int> seg; std::vector<double> cs;
            twin.current(seg, cs);
            std::vector<double> got((size_t)B * N * SOLVER_NP), got_state(st.size()), got_bw((size_t)Q * 2 * S * 8);
            if (tmpc_debug_get_params(h, got.data())) { std::printf("%s\n", tmpc_last_error(h)); return 1; }
            if (hipMemcpy(got_state.data(), d_state, got_state.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return 1;
            if (hipMemcpy(got_bw.data(), twin.boundWindow(), got_bw.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return 1;
            std::vector<double> want = start, want_state = st;
            for (int q = 0; q < Q; q++) {
                int hs = tick == 0 ? -1 : seg[q]; double s = 0.;
                struct P { double x, y; double operator()(int i) const { return i ? y : x; } } p{pos[q][0], pos[q][1]};
                paths[q].findClosestPoint(p, hs, s);
                segment_differ += hs != seg[q] || std::memcmp(&s, &cs[q], 8) != 0;
                std::vector<PathSegment> win, left, right;
                paths[q].window(hs, S, win, &left, &right);
                for (int side = 0; side < 2; side++)
                    for (int w = 0; w < S; w++) {
                        const PathSegment &c = side ? right[w] : left[w];
                        const double v[8] = {c.ax, c.bx, c.cx, c.dx, c.ay, c.by, c.cy, c.dy};
                        bound_differ += std::memcmp(v, &got_bw[(((size_t)q * 2 + side) * S + w) * 8], 64) != 0;
                    }
                for (int b = 0; b < B; b++) {
                    if (scene_of[b] != q) continue;
                    want_state[(size_t)b * SOLVER_NX + 4] = s;
                    for (int k = 0; k < N; k++) {                                // the host's setSplineParameters into a scratch solver row
                        AcadosParameters &pr = solver->_params;
                        for (int i = 0; i < SOLVER_NP; i++) pr.all_parameters[k * SOLVER_NP + i] = -7.;
                        for (int i = 0; i < S; i++) {
                            const PathSegment &sg = win[i];
                            setSolverParameterSplineXA(k, pr, sg.ax, i); setSolverParameterSplineXB(k, pr, sg.bx, i); setSolverParameterSplineXC(k, pr, sg.cx, i);
                            setSolverParameterSplineXD(k, pr, sg.dx, i); setSolverParameterSplineYA(k, pr, sg.ay, i); setSolverParameterSplineYB(k, pr, sg.by, i);
                            setSolverParameterSplineYC(k, pr, sg.cy, i); setSolverParameterSplineYD(k, pr, sg.dy, i); setSolverParameterSplineStart(k, pr, sg.start, i);
                        }
                        for (int i = 0; i < SOLVER_NP; i++) want[((size_t)b * N + k) * SOLVER_NP + i] = pr.all_parameters[k * SOLVER_NP + i];
                    }
                }
            }
            for (size_t i = 0; i < got.size(); i++) { differ += std::memcmp(&got[i], &want[i], 8) != 0; written += tick == 0 && want[i] != -7.; }
            for (size_t i = 0; i < st.size(); i++) state_differ += std::memcmp(&got_state[i], &want_state[i], 8) != 0;
            std::printf("batch_tick %d segments %d %d\n", tick, seg[0], seg[1]);
        }
        std::printf("batch differ %zu written %zu state_differ %zu bound_differ %zu segment_differ %d\n", differ, written, state_differ, bound_differ, segment_differ);
    }
    (void)hipFree(d_pos); (void)hipFree(d_state);
    tmpc_destroy(h);
    return 0;
}
#endif
