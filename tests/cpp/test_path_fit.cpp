// Waypoints -> cubic segments in C++ (mpc_planner_modules/reference_path.h: fit / fitBounds / fitCubic -- DESIGN.md U15).
// Two programs from this file, both driven by tests/test_cpp_path_fit.py:
//   (default)            Solver-free, g++ only, CPU:  test_path_fit <scenes.bin>
//       scenes.bin: n_scenes n_pts_max given_s extras; per scene: count, n_pts_max x 2 waypoints, n_pts_max s, 2 x n_pts_max x 2 bound waypoints
//       (left, right), n_pts_max v.  Prints per scene "scene q status count length road_width" and, for a fitted scene, "p q i 9 numbers", with
//       extras "l q i 8 numbers", "r q i 8 numbers", "v q i 4 numbers" -- %.17g round-trips a double.
//   -DWITH_SOLVER         against a generated solver's headers:  test_path_fit_solver contouring <config dir> <scene.bin>  (CPU: no Solver object is made)
//       scene.bin: S; px py; n; n x 2 waypoints, n x 2 left, n x 2 right.  Contouring::onDataReceived with waypoints followed by update against
//       fit followed by window ("contouring differ 0 ..."), the bounds and road width with road constraints on ("bounds differ 0 ..."), and
//       onDataReceived without waypoints, which must leave data as it is ("untouched 1").
//                          test_path_fit_solver batch <config dir> <scene.bin>  (needs a GPU)
//       the batched device twin (reference_path_batch.h): setWaypoints followed by a tick against setPaths with host-fitted cubics followed by
//       the same tick, bitwise ("batch differ 0 ...").
#ifdef WITH_SOLVER
#include <mpc_planner_modules/modules_hip.h>
#include <mpc_planner_modules/reference_path_batch.h>
#include <cstring>
#include <string>
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
static void print_segment(char tag, int q, size_t i, const PathSegment &c, bool with_start)
{
    std::printf("%c %d %zu %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g", tag, q, i, c.ax, c.bx, c.cx, c.dx, c.ay, c.by, c.cy, c.dy);
    if (with_start) std::printf(" %.17g", c.start);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::vector<double> in = read_all(argv[1]);
    size_t o = 0;
    auto next = [&]() { return in.at(o++); };
    const int n_scenes = (int)next(), P = (int)next(), given_s = (int)next(), extras = (int)next();
    for (int q = 0; q < n_scenes; q++) {
        int count = (int)next();
        count = count < 0 ? 0 : (count > P ? P : count);
        const size_t xy_at = o, s_at = xy_at + (size_t)P * 2, left_at = s_at + P, right_at = left_at + (size_t)P * 2, v_at = right_at + (size_t)P * 2;
        o = v_at + P;
        std::vector<double> x(count), y(count), s, lx(count), ly(count), rx(count), ry(count), v(count);
        for (int i = 0; i < count; i++) {
            x[i] = in[xy_at + 2 * i]; y[i] = in[xy_at + 2 * i + 1];
            lx[i] = in[left_at + 2 * i]; ly[i] = in[left_at + 2 * i + 1]; rx[i] = in[right_at + 2 * i]; ry[i] = in[right_at + 2 * i + 1];
            v[i] = in[v_at + i];
            if (given_s) s.push_back(in[s_at + i]);
        }
        ReferencePathSpline path;
        const bool ok = path.fit(x, y, s);
        double width = -3.0;
        if (ok && extras && !path.fitBounds(lx, ly, rx, ry, &width)) { std::printf("fitBounds failed on scene %d\n", q); return 1; }
        std::printf("scene %d %d %zu %.17g %.17g\n", q, ok ? 0 : 1, path.segments.size(), path.length, width);
        if (!ok) continue;
        for (size_t i = 0; i < path.segments.size(); i++) print_segment('p', q, i, path.segments[i], true);
        if (extras) {
            for (size_t i = 0; i < path.left_bound.size(); i++) print_segment('l', q, i, path.left_bound[i], false);
            for (size_t i = 0; i < path.right_bound.size(); i++) print_segment('r', q, i, path.right_bound[i], false);
            std::vector<double> a, b, c, d;
            if (!ReferencePathSpline::fitCubic(path.t_vector, v, a, b, c, d)) { std::printf("fitCubic failed on scene %d\n", q); return 1; }
            for (size_t i = 0; i < a.size(); i++) std::printf("v %d %zu %.17g %.17g %.17g %.17g\n", q, i, a[i], b[i], c[i], d[i]);
        }
    }
    return 0;
}
#else
static bool same(const PathSegment &a, const PathSegment &b) { return std::memcmp(&a, &b, sizeof(PathSegment)) == 0; }
static size_t differ(const std::vector<PathSegment> &a, const std::vector<PathSegment> &b)
{
    size_t n = a.size() != b.size() ? 1 : 0;
    for (size_t i = 0; i < a.size() && i < b.size(); i++) n += same(a[i], b[i]) ? 0 : 1;
    return n;
}

struct Scene { int S; double px, py; ReferencePath path; Boundary left, right; };
static Scene read_scene(const char *file)
{
    const std::vector<double> in = read_all(file);
    size_t o = 0;
    auto next = [&]() { return in.at(o++); };
    Scene sc;
    sc.S = (int)next(); sc.px = next(); sc.py = next();
    const int n = (int)next();
    for (Boundary *b : {&sc.path, &sc.left, &sc.right})
        for (int i = 0; i < n; i++) { b->x.push_back(next()); b->y.push_back(next()); }
    return sc;
}

static int contouring(const Scene &sc)
{
    ModuleConfig cfg;
    cfg.num_segments = sc.S;
    ReferencePathSpline want;
    double want_width = 0.;
    if (!want.fit(sc.path.x, sc.path.y) || !want.fitBounds(sc.left.x, sc.left.y, sc.right.x, sc.right.y, &want_width)) return 1;
    State state;
    state.set("x", sc.px); state.set("y", sc.py);
    {   // waypoints, no road constraints: onDataReceived fits, update tracks the fitted path (no Solver is touched on this way)
        RealTimeData data;
        data.reference_path_points = sc.path;
        Contouring module(nullptr, cfg);
        ModuleData module_data;
        module.onDataReceived(data, "reference_path");
        module.update(state, data, module_data);
        int segment = -1; double s = 0.;
        want.findClosestPoint(state.getPos(), segment, s, cfg.path_search_range);
        std::vector<PathSegment> window;
        want.window(segment, sc.S, window);
        const double got_s = state.get("spline");
        std::printf("contouring differ %zu path_differ %zu segment %d %d spline_same %d length_same %d bounds %zu %zu width_same %d\n", differ(module_data.path, window),
                    differ(data.reference_path, want.segments), module_data.current_path_segment, segment, (int)(std::memcmp(&got_s, &s, 8) == 0),
                    (int)(data.reference_path_length == want.length), data.left_bound.size(), data.right_bound.size(), (int)(module.roadWidth() == cfg.road_width));
    }
    {   // road constraints on and both bounds' waypoints: the bound curves on the centreline's knots, road/width from their first waypoints
        cfg.add_road_constraints = true;
        RealTimeData data;
        data.reference_path_points = sc.path; data.left_bound_points = sc.left; data.right_bound_points = sc.right;
        Contouring module(nullptr, cfg);
        module.onDataReceived(data, "reference_path");
        const double w = module.roadWidth();
        std::printf("bounds differ %zu %zu width_same %d width %.17g\n", differ(data.left_bound, want.left_bound), differ(data.right_bound, want.right_bound),
                    (int)(std::memcmp(&w, &want_width, 8) == 0), w);
    }
    {   // no waypoints: the cubics arrive fitted, data stays as it is
        RealTimeData data;
        data.reference_path = want.segments; data.reference_path_length = 12.5; data.left_bound = want.right_bound; data.right_bound = want.left_bound;
        Contouring module(nullptr, cfg);
        module.onDataReceived(data, "reference_path");
        const bool untouched = differ(data.reference_path, want.segments) == 0 && data.reference_path_length == 12.5 && differ(data.left_bound, want.right_bound) == 0 &&
                               differ(data.right_bound, want.left_bound) == 0 && data.reference_path_points.empty() && module.roadWidth() == cfg.road_width;
        std::printf("untouched %d\n", (int)untouched);
    }
    return 0;
}

static std::vector<double> download(const void *d, size_t n_doubles)
{
    std::vector<double> v(n_doubles);
    if (hipMemcpy(v.data(), d, n_doubles * 8, hipMemcpyDeviceToHost) != hipSuccess) { std::printf("hipMemcpy failed\n"); std::exit(1); }
    return v;
}

// three scenes: the whole path with bounds, its first four waypoints (three segments, fewer than S: padded slots), and one with a repeated
// waypoint (invalid: count 0, the tick leaves it alone)
static int batch(const Scene &sc)
{
    const int Q = 3, S = sc.S, R = (int)sc.path.x.size() + 2;             // (a row stride larger than the longest path)
    std::vector<ReferencePath> pts(Q);
    std::vector<Boundary> left(Q), right(Q);
    for (int q = 0; q < Q; q++) {
        const size_t n = q == 1 ? 4 : sc.path.x.size();
        for (auto pr : {std::make_pair(&pts[q], &sc.path), std::make_pair(&left[q], &sc.left), std::make_pair(&right[q], &sc.right)}) {
            pr.first->x.assign(pr.second->x.begin(), pr.second->x.begin() + n); pr.first->y.assign(pr.second->y.begin(), pr.second->y.begin() + n);
        }
    }
    pts[2].x[5] = pts[2].x[4]; pts[2].y[5] = pts[2].y[4];
    std::vector<ReferencePathSpline> fitted(Q);
    std::vector<double> width(Q, 0.);
    for (int q = 0; q < Q; q++)
        if (fitted[q].fit(pts[q].x, pts[q].y)) fitted[q].fitBounds(left[q].x, left[q].y, right[q].x, right[q].y, &width[q]);
    if (fitted[0].empty() || fitted[1].numSegments() != 3 || !fitted[2].empty()) { std::printf("unexpected host fit\n"); return 1; }
    tmpc_dims d;
    tmpc_default_dims_ex(&d, SOLVER_N, SOLVER_S, SOLVER_NLIN, SOLVER_M, SOLVER_NSLK, SOLVER_SLACK);
    tmpc_handle *h = nullptr;
    if (tmpc_create(&h, &d, 4, 0)) { std::printf("tmpc_create failed\n"); return 1; }
    const double pos[Q][2] = {{sc.px, sc.py}, {sc.path.x[2] + 0.1, sc.path.y[2] - 0.2}, {sc.px, sc.py}};
    void *d_pos = nullptr;
    if (hipMalloc(&d_pos, sizeof(pos)) != hipSuccess || hipMemcpy(d_pos, pos, sizeof(pos), hipMemcpyHostToDevice) != hipSuccess) return 1;
    {
        BatchedPathTracking from_points(h, Q, R, S, true), from_cubics(h, Q, R, S, true);
        from_points.setWaypoints(pts, &left, &right);
        from_cubics.setPaths(fitted);
        size_t n_differ = 0;
        int segment_differ = 0;
        std::vector<int> seg_a, seg_b; std::vector<double> cs_a, cs_b;
        for (int tick = 0; tick < 2; tick++) {                                   // a global search, then a local one
            from_points.track(d_pos, 2); from_cubics.track(d_pos, 2);
            from_points.current(seg_a, cs_a); from_cubics.current(seg_b, cs_b);
            const std::vector<double> wa = download(from_points.window(), (size_t)Q * S * 9), wb = download(from_cubics.window(), (size_t)Q * S * 9);
            const std::vector<double> ba = download(from_points.boundWindow(), (size_t)Q * 2 * S * 8), bb = download(from_cubics.boundWindow(), (size_t)Q * 2 * S * 8);
            for (int q = 0; q < 2; q++) {                                        // (scene 2 is invalid: nothing of it is written by either twin)
                segment_differ += seg_a[q] != seg_b[q] || std::memcmp(&cs_a[q], &cs_b[q], 8) != 0;
                n_differ += std::memcmp(&wa[(size_t)q * S * 9], &wb[(size_t)q * S * 9], (size_t)S * 9 * 8) != 0;
                n_differ += std::memcmp(&ba[(size_t)q * 2 * S * 8], &bb[(size_t)q * 2 * S * 8], (size_t)2 * S * 8 * 8) != 0;
            }
        }
        // the fitted cubics themselves, the counts, lengths, status and road width
        const std::vector<double> path = download(from_points.paths(), (size_t)Q * R * 9), bounds = download(from_points.bounds(), (size_t)Q * 2 * R * 8);
        const std::vector<double> length = download(from_points.pathLengths(), Q), road = download(from_points.roadWidth(), Q);
        std::vector<int> count(Q); std::vector<unsigned char> status(Q);
        if (hipMemcpy(count.data(), from_points.pathCounts(), Q * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(status.data(), from_points.status(), Q, hipMemcpyDeviceToHost) != hipSuccess) return 1;
        size_t fit_differ = 0;
        for (int q = 0; q < Q; q++) {
            fit_differ += count[q] != fitted[q].numSegments() || status[q] != (fitted[q].empty() ? 1 : 0);
            if (fitted[q].empty()) continue;
            fit_differ += std::memcmp(&length[q], &fitted[q].length, 8) != 0 || std::memcmp(&road[q], &width[q], 8) != 0;
            for (int i = 0; i < count[q]; i++) {
                fit_differ += std::memcmp(&path[((size_t)q * R + i) * 9], &fitted[q].segments[i], 72) != 0;
                fit_differ += std::memcmp(&bounds[(((size_t)q * 2 + 0) * R + i) * 8], &fitted[q].left_bound[i], 64) != 0;
                fit_differ += std::memcmp(&bounds[(((size_t)q * 2 + 1) * R + i) * 8], &fitted[q].right_bound[i], 64) != 0;
            }
        }
        std::printf("batch differ %zu segment_differ %d fit_differ %zu counts %d %d %d segments %d %d %d\n", n_differ, segment_differ, fit_differ, count[0], count[1], count[2],
                    seg_a[0], seg_a[1], seg_a[2]);
    }
    (void)hipFree(d_pos);
    tmpc_destroy(h);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    setSolverConfigPath(argv[2]);
    const Scene sc = read_scene(argv[3]);
    if (sc.S != SOLVER_S) { std::printf("scene does not match the generated solver\n"); return 2; }
    return std::string(argv[1]) == "batch" ? batch(sc) : contouring(sc);
}
#endif
