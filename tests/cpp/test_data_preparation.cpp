// C++ obstacle preparation (mpc_planner/data_preparation.h: the reference's mpc_planner/src/data_preparation.cpp on the Eigen-free types) on a raw
// obstacle list written by tests/test_cpp_data_preparation.py, the way a wrapper's obstacle callback runs it:
//   constant-velocity mode (ros1_jackal.cpp:313-332): getConstantVelocityPrediction per obstacle, [removeDistantObstacles,] ensureObstacleSize,
//       propagatePredictionUncertainty -- in probabilistic mode two uncertainty passes in all;
//   given mode (ros1_jackalsimulator.cpp:298-347): predictions as given, GAUSSIAN iff probabilistic and the last step's major != 0,
//       [removeDistantObstacles,] ensureObstacleSize, one pass if probabilistic/propagate_uncertainty.
//   test_data_preparation <config dir> <scene.bin>        prints the prepared obstacles ("sel", "ob" lines) and the robot area
//   test_data_preparation <config dir> <scene.bin> gpu    also runs the batched twin (mpc_planner/data_preparation_batch.h) on `copies` scenes
//       (the list with 0, drop, 2 drop, .. obstacles dropped from its end) and compares the parameter rows of a batch -- two entries per scene -- that
//       tmpc_set_obstacle_parameters wrote with the rows EllipsoidConstraints::setParameters writes from the host-prepared obstacles: "rows" line.
// Scene: n, given, probabilistic, propagate_uncertainty, max_obstacle_distance, copies, drop; x y psi v; per obstacle x y vx vy radius; given: n x N x 5.
#include <mpc_planner/data_preparation_batch.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    setSolverConfigPath(argv[1]);
    const bool gpu = argc > 3 && !std::strcmp(argv[3], "gpu");
    const std::vector<double> in = read_all(argv[2]);
    size_t o = 0;
    auto next = [&]() { return in[o++]; };
    const int n = (int)next(), given = (int)next();
    ModuleConfig cfg;                                                   // N = SOLVER_N, integrator_step 0.2, max_obstacles 8
    cfg.max_obstacles = SOLVER_MAX_OBSTACLES;
    cfg.probabilistic_enable = next() != 0.; cfg.propagate_uncertainty = next() != 0.; cfg.max_obstacle_distance = next();
    const int copies = (int)next(), drop = (int)next();
    const int N = cfg.N, M = cfg.max_obstacles;
    State state;
    const char *sn[] = {"x", "y", "psi", "v"};
    for (int i = 0; i < 4; i++) state.set(sn[i], next());
    std::vector<DynamicObstacle> raw;
    std::vector<Vector2d> velocity;
    for (int i = 0; i < n; i++) {
        const double x = next(), y = next(), vx = next(), vy = next(), r = next();
        raw.emplace_back(i, Vector2d(x, y), 0., r);
        velocity.emplace_back(vx, vy);
    }
    if (given)
        for (int i = 0; i < n; i++) {
            raw[i].prediction = Prediction(PredictionType::GAUSSIAN);
            for (int k = 0; k < N; k++) { const double x = next(), y = next(), a = next(), ma = next(), mi = next(); raw[i].prediction.modes[0].emplace_back(Vector2d(x, y), a, ma, mi); }
            raw[i].prediction.type = (raw[i].prediction.modes[0].back().major_radius == 0. || !cfg.probabilistic_enable) ? PredictionType::DETERMINISTIC
                                                                                                                      : PredictionType::GAUSSIAN;      // (:331-334)
        }
    // the host path of one scene: the wrapper's callback
    auto host_prepare = [&](std::vector<DynamicObstacle> obstacles, std::vector<int> *selected) {
        if (!given)
            for (size_t i = 0; i < obstacles.size(); i++)
                obstacles[i].prediction = getConstantVelocityPrediction(obstacles[i].position, velocity[i], cfg.integrator_step, cfg.N, cfg);
        std::vector<int> kept(obstacles.size());
        for (size_t i = 0; i < kept.size(); i++) { kept[i] = (int)i; obstacles[i].index = (int)i; }
        if (cfg.max_obstacle_distance > 0.) {
            removeDistantObstacles(obstacles, state, cfg);
            kept.clear();
            for (auto &ob : obstacles) kept.push_back(ob.index);
        }
        std::vector<int> sel;
        ensureObstacleSize(obstacles, state, cfg, &sel);
        if (!given || cfg.propagate_uncertainty) propagatePredictionUncertainty(obstacles, cfg);
        if (selected) { selected->clear(); for (int s : sel) selected->push_back(s < 0 ? -1 : kept[s]); }
        return obstacles;
    };
    const int passes = given ? (cfg.propagate_uncertainty ? 1 : 0) : (cfg.probabilistic_enable ? 2 : 0);      // what the two wrappers amount to
    std::vector<int> selected;
    const std::vector<DynamicObstacle> prepared = host_prepare(raw, &selected);
    std::printf("sel");
    for (int s : selected) std::printf(" %d", s);
    std::printf("\n");
    for (int j = 0; j < M; j++) {
        const DynamicObstacle &ob = prepared[j];
        std::printf("ob %d %d %.17g", j, ob.prediction.type == PredictionType::GAUSSIAN ? 1 : 0, ob.radius);
        for (int k = 0; k < N; k++) { const PredictionStep &st = ob.prediction.modes[0][k]; std::printf(" %.17g %.17g %.17g %.17g %.17g", st.position(0), st.position(1), st.angle, st.major_radius, st.minor_radius); }
        std::printf("\n");
    }
    for (int nd : {1, 3}) {
        std::printf("area %d", nd);
        for (const Disc &d : defineRobotArea(1.0, 0.5, nd)) std::printf(" %.17g %.17g", d.offset, d.radius);
        std::printf("\n");
    }
    if (!gpu) return 0;

    // ---- the batched twin on `copies` scenes against the host path, through the parameter rows ----
    const int Q = copies, B = 2 * Q;
    std::vector<std::vector<DynamicObstacle>> lists;
    for (int q = 0; q < Q; q++) lists.emplace_back(raw.begin(), raw.begin() + std::max(0, n - drop * q));
    std::vector<std::vector<Vector2d>> vels;
    for (int q = 0; q < Q; q++) vels.emplace_back(velocity.begin(), velocity.begin() + std::max(0, n - drop * q));
    RealTimeData data;
    data.robot_area = defineRobotArea(0.65, 0.65, 1);
    ModuleData module_data;
    auto solver = std::make_shared<Solver>(0);
    EllipsoidConstraints ellipsoids(solver, cfg);
    std::vector<double> want((size_t)B * N * SOLVER_NP, -7.), start((size_t)B * N * SOLVER_NP, -7.);
    std::vector<int> scene_of(B), host_selected;
    for (int b = 0; b < B; b++) {
        const int q = b / 2;
        scene_of[b] = q;
        std::vector<int> sel;
        data.dynamic_obstacles = host_prepare(lists[q], &sel);
        host_selected.insert(host_selected.end(), sel.begin(), sel.end());
        for (int i = 0; i < N * SOLVER_NP; i++) solver->_params.all_parameters[i] = -7.;
        ellipsoids.update(state, data, module_data);
        for (int k = 0; k < N; k++) ellipsoids.setParameters(data, module_data, k);
        for (int i = 0; i < N * SOLVER_NP; i++) want[(size_t)b * N * SOLVER_NP + i] = solver->_params.all_parameters[i];
    }
    tmpc_dims d;
    tmpc_default_dims_ex(&d, SOLVER_N, SOLVER_S, SOLVER_NLIN, SOLVER_M, SOLVER_NSLK, SOLVER_SLACK);
    tmpc_handle *h = nullptr;
    if (tmpc_create(&h, &d, B, 0)) { std::printf("tmpc_create failed\n"); return 1; }
    std::vector<double> xinit((size_t)B * SOLVER_NX, 0.), x0((size_t)B * (N + 1) * (SOLVER_NX + SOLVER_NU), 0.);
    if (tmpc_set_batch(h, B, xinit.data(), x0.data(), start.data())) { std::printf("%s\n", tmpc_last_error(h)); return 1; }
    {
        BatchedObstaclePreparation twin(h, Q, n, cfg);
        twin.prepare(lists, std::vector<State>(Q, state), given ? nullptr : &vels, passes);
        twin.setParameters(scene_of);
        std::vector<double> got((size_t)B * N * SOLVER_NP);
        if (tmpc_debug_get_params(h, got.data())) { std::printf("%s\n", tmpc_last_error(h)); return 1; }
        size_t differ = 0, written = 0;
        for (size_t i = 0; i < got.size(); i++) { differ += std::memcmp(&got[i], &want[i], 8) != 0; written += want[i] != -7.; }
        const std::vector<int> dev_sel = twin.selected();
        size_t sel_differ = 0;
        for (int b = 0; b < B; b++) for (int j = 0; j < M; j++) sel_differ += dev_sel[(size_t)(b / 2) * M + j] != host_selected[(size_t)b * M + j];
        std::printf("rows scenes %d entries %d written %zu differ %zu selected_differ %zu\n", Q, B, written, differ, sel_differ);
    }
    tmpc_destroy(h);
    return 0;
}
