// PathReferenceVelocity in C++ (mpc_planner_modules/modules_hip.h; PathVelocityProfile of reference_path.h -- DESIGN.md U15, U17) against the
// numpy mirror, driven by tests/test_cpp_path_velocity.py.  CPU: built against the host side of a generated stack that has the spline_v
// columns; no Solver object is made and nothing touches a GPU.
//   test_path_velocity <config dir> <scene.bin>
//   scene.bin: S; reference_velocity; given_s; n; n x (x y s v); n_ticks; per tick: segment, s.
// Prints "profile <segments> <length>", per tick "tick t v_ref" and "p t k <SOLVER_NP numbers>" for k = 0 and N - 1 -- the parameter rows
// after setParameters on a block prefilled with -3 --, then "noprofile k <numbers>" for a path without velocities and "published 0|1" twice:
// whether update() put a profile into ModuleData (%.17g round-trips a double).
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

static void print_row(const char *tag, int t, int k, const AcadosParameters &params)
{
    if (t >= 0) std::printf("%s %d %d", tag, t, k); else std::printf("%s %d", tag, k);
    for (int i = 0; i < SOLVER_NP; i++) std::printf(" %.17g", params.all_parameters[k * SOLVER_NP + i]);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    setSolverConfigPath(argv[1]);
    const std::vector<double> in = read_all(argv[2]);
    size_t at = 0;
    auto next = [&]() { return in.at(at++); };
    ModuleConfig cfg;
    cfg.num_segments = (int)next();
    cfg.weights["reference_velocity"] = next();
    const bool given_s = next() != 0.;
    const int n = (int)next();
    RealTimeData data;
    for (int i = 0; i < n; i++) {
        data.reference_path_points.x.push_back(next()); data.reference_path_points.y.push_back(next());
        const double s = next();
        if (given_s) data.reference_path_points.s.push_back(s);
        data.reference_path_points.v.push_back(next());
    }
    State state;
    PathReferenceVelocity module(nullptr, cfg);
    ModuleData module_data;
    module.onDataReceived(data, "reference_path");
    module.update(state, data, module_data);
    std::printf("published %d\n", (int)(module_data.path_velocity != nullptr));
    if (module_data.path_velocity) std::printf("profile %d %.17g\n", module_data.path_velocity->numSegments(), module_data.path_velocity->length);
    const int n_ticks = (int)next();
    for (int t = 0; t < n_ticks; t++) {
        module_data.current_path_segment = (int)next();
        const double s = next();
        AcadosParameters params;
        for (double &p : params.all_parameters) p = -3.0;
        for (int k = 0; k < SOLVER_N; k++) module.setParameters(params, data, module_data, k);
        std::printf("tick %d %.17g\n", t, module_data.path_velocity ? (*module_data.path_velocity)(s) : cfg.weights.at("reference_velocity"));
        print_row("p", t, 0, params); print_row("p", t, SOLVER_N - 1, params);
    }
    {   // a path without velocities: no profile is published, every slot is (0, 0, 0, reference_velocity)
        RealTimeData plain;
        plain.reference_path_points = data.reference_path_points; plain.reference_path_points.v.clear();
        PathReferenceVelocity none(nullptr, cfg);
        ModuleData md;
        none.onDataReceived(plain, "reference_path");
        none.update(state, plain, md);
        std::printf("published %d\n", (int)(md.path_velocity != nullptr));
        md.current_path_segment = 1;
        AcadosParameters params;
        for (double &p : params.all_parameters) p = -3.0;
        for (int k = 0; k < SOLVER_N; k++) none.setParameters(params, plain, md, k);
        print_row("noprofile", -1, SOLVER_N - 1, params);
    }
    return 0;
}
