// C++ end-to-end of the road constraints (contouring.cpp:181-262 restated in mpc_planner_modules/modules_hip.h): Contouring::update fills
// ModuleData::static_obstacles from the main solver's warm start, LinearizedConstraints appends the two halfspaces behind the obstacle rows
// of every planner of the batched GuidanceConstraints::optimize -- on a scene written by tests/test_cpp_road.py, for a solver generated with
// add_halfspaces=2 (SOLVER_NLIN = SOLVER_MAX_OBSTACLES + 2).  Prints what tests/cpp/test_optimize.cpp prints, plus the halfspaces themselves.
//   test_road_constraints <config dir> <scene.bin>
// Scene: N M B S tmpcpp; 8 weights; robot radius, obstacle radius; state; per obstacle N x (x, y); S x 9 path segments; per trajectory the
// guidance positions and velocities; previously selected; road mode (0: add_road_constraints = false, 1: centreline, 2: bounds), road/width,
// road/two_way; mode 2: S x 8 left-bound and S x 8 right-bound coefficients.
#include <mpc_planner_modules/modules_hip.h>

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

int main(int argc, char **argv)
{
    static_assert(SOLVER_NLIN == SOLVER_MAX_OBSTACLES + 2, "generate the solver with add_halfspaces=2");
    if (argc < 3) return 2;
    setSolverConfigPath(argv[1]);
    const std::vector<double> in = read_all(argv[2]);
    size_t o = 0;
    auto next = [&]() { return in[o++]; };
    const int N = (int)next(), M = (int)next(), B = (int)next(), S = (int)next(), tmpcpp = (int)next();
    if (N != SOLVER_N || M != SOLVER_MAX_OBSTACLES || S != SOLVER_S) { std::printf("scene does not match the generated solver\n"); return 2; }
    ModuleConfig cfg;
    cfg.max_obstacles = M; cfg.num_segments = S; cfg.n_paths = B; cfg.use_tmpcpp = tmpcpp != 0;
    cfg.n_other_halfspaces = SOLVER_NLIN - SOLVER_MAX_OBSTACLES;                // linearized_constraints/add_halfspaces: 2
    const char *wn[] = {"acceleration", "angular_velocity", "velocity", "reference_velocity", "contour", "lag", "terminal_angle", "terminal_contouring"};
    for (int i = 0; i < 8; i++) cfg.weights[wn[i]] = next();
    cfg.robot_radius = next();
    const double obstacle_radius = next();
    State state;
    const char *sn[] = {"x", "y", "psi", "v", "spline"};
    for (int i = 0; i < 5; i++) state.set(sn[i], next());
    RealTimeData data;
    data.robot_area.emplace_back(0., cfg.robot_radius);
    for (int j = 0; j < M; j++) {
        DynamicObstacle ob(j, Vector2d(0., 0.), 0., obstacle_radius);
        ob.prediction = Prediction(PredictionType::DETERMINISTIC);
        for (int i = 0; i < N; i++) { const double x = next(), y = next(); ob.prediction.modes[0].emplace_back(Vector2d(x, y), 0., 0., 0.); }
        ob.position = ob.prediction.modes[0][0].position;
        data.dynamic_obstacles.push_back(ob);
    }
    ModuleData module_data;
    auto segment = [&](bool with_start) {
        PathSegment sg;
        sg.ax = next(); sg.bx = next(); sg.cx = next(); sg.dx = next(); sg.ay = next(); sg.by = next(); sg.cy = next(); sg.dy = next();
        sg.start = with_start ? next() : 0.;
        return sg;
    };
    for (int i = 0; i < S; i++) module_data.path.push_back(segment(true));
    std::vector<GuidanceTrajectory> guidance(B);
    for (int b = 0; b < B; b++) {
        guidance[b].topology_class = b;
        for (int k = 0; k <= N; k++) { const double x = next(), y = next(); guidance[b].positions.emplace_back(x, y); }
        for (int k = 0; k <= N; k++) { const double x = next(), y = next(); guidance[b].velocities.emplace_back(x, y); }
    }
    const int selected_before = (int)next();
    if (selected_before >= 0) guidance[selected_before].previously_selected = true;
    const int road_mode = (int)next();
    cfg.add_road_constraints = road_mode != 0;
    cfg.road_width = next();
    cfg.two_way_road = next() != 0.;
    if (road_mode == 2) {
        for (int i = 0; i < S; i++) data.left_bound.push_back(segment(false));
        for (int i = 0; i < S; i++) data.right_bound.push_back(segment(false));
    }

    // main solver: Planner::solveMPC's preparation (planner.cpp:64-113): xinit, forward-propagated warm start, objective modules
    auto solver = std::make_shared<Solver>(0);
    solver->setXinit(state);
    solver->_config["deceleration_at_infeasible"] = 0.0;
    solver->initializeWithBraking(state);
    MPCBaseModule base(solver, cfg, {"acceleration", "angular_velocity", "velocity", "reference_velocity"});
    Contouring contouring(solver, cfg);
    contouring.update(state, data, module_data);                                // -> module_data.static_obstacles (road constraints)
    for (int k = 0; k < N; k++) { base.setParameters(data, module_data, k); contouring.setParameters(data, module_data, k); }
    for (size_t k = 0; k < module_data.static_obstacles.size(); k++) {
        std::printf("road %zu", k);
        for (const auto &hs : module_data.static_obstacles[k]) std::printf(" %.17g %.17g %.17g", hs.A(0), hs.A(1), hs.b);
        std::printf("\n");
    }

    GuidanceConstraints guidance_constraints(solver, cfg);
    guidance_constraints.setGuidanceTrajectories(guidance);
    const int exit_code = guidance_constraints.optimize(state, data, module_data);
    std::printf("exit_code %d best %d\n", exit_code, guidance_constraints.best_planner_index_);
    for (auto &pl : guidance_constraints.planners_)
        std::printf("planner %d disabled %d exit %d objective %.17g guidance_id %d\n", pl.id, (int)pl.disabled, pl.result.exit_code, pl.result.objective, pl.result.guidance_ID);
    for (int k = 0; k <= N; k++)
        std::printf("x %d %.17g %.17g %.17g %.17g %.17g\n", k, solver->getOutput(k, "x"), solver->getOutput(k, "y"), solver->getOutput(k, "psi"),
                    solver->getOutput(k, "v"), solver->getOutput(k, "spline"));
    // the parameter rows every planner was solved with (q = planner), then the best planner's, copied into the main solver
    for (auto &pl : guidance_constraints.planners_)
        for (int k = 0; k < N; k++) {
            std::printf("q %d %d", pl.id, k);
            for (int i = 0; i < SOLVER_NP; i++) std::printf(" %.17g", pl.local_solver->_params.all_parameters[k * SOLVER_NP + i]);
            std::printf("\n");
        }
    for (int k = 0; k < N; k++) {
        std::printf("p %d", k);
        for (int i = 0; i < SOLVER_NP; i++) std::printf(" %.17g", solver->_params.all_parameters[k * SOLVER_NP + i]);
        std::printf("\n");
    }
    // RealTimeData::reset() clears the per-tick road bounds like the reference's (realtime_data.h:37-47) and keeps the disc model
    data.reset();
    std::printf("reset %zu %zu %zu\n", data.left_bound.size(), data.right_bound.size(), data.robot_area.size());
    return 0;
}
