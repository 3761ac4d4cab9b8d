// The guidance hand-off in C++ (mpc_planner_modules/guidance_handoff.h: GuidanceSpline, guidancePlan, guidanceDecide; guidance_handoff_batch.h:
// BatchedGuidanceHandoff -- DESIGN.md U18), driven by tests/test_cpp_guidance_handoff.py.
//   test_guidance_handoff host <case.bin>     CPU: the Solver-free header alone; nothing touches a GPU
//   test_guidance_handoff device <case.bin>   GPU: the batched twin next to the same calls made through the C-ABI with buffers of the program's own
// case.bin (doubles): N dt R n_paths use_tmpcpp warmstart shift weight explicit Q ticks nx deceleration control_dt; state [Q][nx];
//   host:   xtraj [B][(N + 1) nx]; utraj [B][N 2]
//   device: S n_lin M npar; xinit [B][nx]; x0 [B][(N + 1)(nx + 2)]; params [B][N npar]   (the batch is set and solved once)
//   per tick: enable_output; counts [Q]; per scene and path: class, previously_selected, node count, R x (t x y);  host: pobj [B]; code [B]
// Prints per tick "tick t" and one line "<name> <numbers>" per array (%.17g round-trips a double): mode src init_enabled rows_dummy disabled
// guidance_id weight status gpos gvel pobj code v1 w0 best exit cmd ids sel; device: also "equal 0|1" -- the twin's buffers against the
// C-ABI path's, byte for byte.
#include <mpc_planner_modules/guidance_handoff_batch.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

template <class T> static void line(const char *name, const std::vector<T> &v)
{
    std::printf("%s", name);
    for (const T &x : v) std::printf(" %.17g", (double)x);
    std::printf("\n");
}

#define HIP_OK(expr) do { if ((expr) != hipSuccess) { std::printf("HIP error: %s\n", #expr); std::exit(3); } } while (0)
#define TMPC_OK_(expr, h) do { if ((expr) != 0) { std::printf("%s: %s\n", #expr, tmpc_last_error(h)); std::exit(3); } } while (0)

template <class T> static std::vector<T> down(const void *d, size_t n)
{
    std::vector<T> v(n);
    HIP_OK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}
template <class T> static void *up(const std::vector<T> &v)
{
    void *d = nullptr;
    HIP_OK(hipMalloc(&d, v.size() * sizeof(T) + 8));
    HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0; }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const bool device = std::string(argv[1]) == "device";
    const std::vector<double> in = read_all(argv[2]);
    size_t at = 0;
    auto next = [&]() { return in.at(at++); };
    auto take = [&](size_t n) { std::vector<double> v(in.begin() + at, in.begin() + at + n); at += n; return v; };
    const int N = (int)next(); double dt = next(); const int R = (int)next();
    GuidanceHandoffConfig cfg;
    cfg.n_paths = (int)next(); cfg.use_tmpcpp = next() != 0.; cfg.warmstart_with_mpc_solution = next() != 0.; cfg.shift_previous_solution_forward = next() != 0.;
    cfg.selection_weight_consistency = next();
    const bool explicit_prev = next() != 0.;
    const int Q = (int)next(), ticks = (int)next(), nx = (int)next();
    const double deceleration = next(), control_dt = next();
    const int P = cfg.P(), B = Q * P;
    const std::vector<double> state = take((size_t)Q * nx);
    std::vector<double> xtraj, utraj;
    tmpc_handle *h = nullptr;
    void *d_state = nullptr;
    if (!device) { xtraj = take((size_t)B * (N + 1) * nx); utraj = take((size_t)B * N * 2); }
    else {
        const int S = (int)next(), n_lin = (int)next(), M = (int)next(), npar = (int)next();
        tmpc_dims dims;
        tmpc_default_dims(&dims, N, S, n_lin, M);
        if (dims.npar != npar) { std::printf("npar %d != %d\n", dims.npar, npar); return 3; }
        dt = dims.dt;
        if (tmpc_create(&h, &dims, B, 0)) { std::printf("tmpc_create failed\n"); return 3; }
        const std::vector<double> xinit = take((size_t)B * nx), x0 = take((size_t)B * (N + 1) * (nx + 2)), params = take((size_t)B * N * npar);
        TMPC_OK_(tmpc_set_batch(h, B, xinit.data(), x0.data(), params.data()), h);
        TMPC_OK_(tmpc_solve(h), h);
        xtraj.assign((size_t)B * (N + 1) * nx, 0.); utraj.assign((size_t)B * N * 2, 0.);
        TMPC_OK_(tmpc_get(h, xtraj.data(), utraj.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), h);
        d_state = up(state);
    }
    GuidanceHandoffState host_state;
    host_state.reset(Q, P);
    BatchedGuidanceHandoff *twin = device ? new BatchedGuidanceHandoff(h, Q, cfg, R, N) : nullptr;
    void *c_ids = nullptr, *c_sel = nullptr;                            // the C-ABI path's own state
    if (device) { c_ids = up(host_state.planner_ids); c_sel = up(host_state.selection); }
    tmpc_guidance_options opt{};
    opt.size = sizeof(opt); opt.n_paths = cfg.n_paths; opt.use_tmpcpp = cfg.use_tmpcpp; opt.warmstart_with_mpc_solution = cfg.warmstart_with_mpc_solution;
    opt.shift_previous_solution_forward = cfg.shift_previous_solution_forward; opt.selection_weight_consistency = cfg.selection_weight_consistency;
    const size_t K = (size_t)N + 1;
    for (int t = 0; t < ticks; t++) {
        const bool enable_output = next() != 0.;
        std::vector<int32_t> counts(Q), classes((size_t)Q * cfg.n_paths), node_count(B, 0);
        std::vector<uint8_t> prev((size_t)Q * cfg.n_paths);
        std::vector<double> nodes((size_t)B * R * 3, 0.);
        std::vector<std::vector<GuidanceCandidate>> guidance(Q);
        for (int q = 0; q < Q; q++) counts[q] = (int)next();
        for (int q = 0; q < Q; q++)
            for (int i = 0; i < cfg.n_paths; i++) {
                GuidanceCandidate g;
                g.topology_class = (int)next(); g.previously_selected = next() != 0.;
                const int n = (int)next();
                const std::vector<double> raw = take((size_t)R * 3);
                for (int j = 0; j < n && j < R; j++) g.nodes.push_back(GuidanceNode{raw[j * 3], raw[j * 3 + 1], raw[j * 3 + 2]});
                classes[(size_t)q * cfg.n_paths + i] = g.topology_class; prev[(size_t)q * cfg.n_paths + i] = g.previously_selected;
                if (i < counts[q]) {                                    // the twin sees the trajectories the search found; the others have no nodes
                    guidance[q].push_back(g);
                    node_count[(size_t)q * P + i] = n;
                    std::memcpy(&nodes[((size_t)q * P + i) * R * 3], raw.data(), (size_t)R * 3 * 8);
                }
            }
        std::printf("tick %d\n", t);
        std::vector<double> pobj, gpos((size_t)B * K * 2), gvel((size_t)B * K * 2);
        std::vector<int32_t> code, status(B);
        GuidancePlan plan;
        GuidanceDecision dec;
        if (!device) {
            pobj = take(B);
            for (double c : take(B)) code.push_back((int32_t)c);
            guidancePlan(cfg, Q, counts.data(), classes.data(), explicit_prev ? prev.data() : nullptr, host_state, plan);
            for (int b = 0; b < B; b++) {
                GuidanceSpline spline;
                std::vector<GuidanceNode> list;
                for (int j = 0; j < node_count[b]; j++) list.push_back(GuidanceNode{nodes[((size_t)b * R + j) * 3], nodes[((size_t)b * R + j) * 3 + 1], nodes[((size_t)b * R + j) * 3 + 2]});
                spline.fit(list, R);
                std::vector<double> pos, vel;
                status[b] = spline.sample(N, dt, pos, vel);
                std::memcpy(&gpos[(size_t)b * K * 2], pos.data(), K * 2 * 8); std::memcpy(&gvel[(size_t)b * K * 2], vel.data(), K * 2 * 8);
            }
            guidanceDecide(cfg, Q, pobj.data(), code.data(), plan, state.data(), xtraj.data(), utraj.data(), N, nx, 2, deceleration, control_dt, enable_output, host_state, dec);
        } else {
            // ---- the twin
            twin->setGuidance(guidance, explicit_prev);
            twin->plan(); twin->sample(); twin->decide(d_state, deceleration, control_dt, enable_output);
            TMPC_OK_(tmpc_synchronize(h), h);
            plan.mode = down<int32_t>(twin->mode(), B); plan.src = down<int32_t>(twin->src(), B); plan.guidance_id = down<int32_t>(twin->guidanceId(), B);
            plan.init_enabled = down<uint8_t>(twin->initEnabled(), B); plan.rows_dummy = down<uint8_t>(twin->rowsDummy(), B); plan.disabled = down<uint8_t>(twin->disabled(), B);
            plan.weight = down<double>(twin->weight(), B);
            gpos = down<double>(twin->positions(), gpos.size()); gvel = down<double>(twin->velocities(), gvel.size()); status = down<int32_t>(twin->status(), B);
            dec.best = down<int32_t>(twin->best(), Q); dec.exit_code = down<int32_t>(twin->exitCode(), Q); dec.cmd = down<double>(twin->cmd(), (size_t)Q * 2);
            host_state.planner_ids = down<int32_t>(twin->plannerIds(), B); host_state.selection = down<int32_t>(twin->selection(), (size_t)Q * 3);
            void *d_pobj = nullptr, *d_code = nullptr;
            TMPC_OK_(tmpc_result_device_ptrs(h, &d_pobj, &d_code), h);
            pobj = down<double>(d_pobj, B); code = down<int32_t>(d_code, B);
            // ---- the same through the C-ABI, buffers of the program's own
            void *c_nodes = up(nodes), *c_ncount = up(node_count), *c_counts = up(counts), *c_classes = up(classes), *c_prev = up(prev);
            std::vector<int32_t> zi(B, -9); std::vector<uint8_t> zu(B, 9); std::vector<double> zd(B, -9.), zg(gpos.size(), -9.);
            void *c_mode = up(zi), *c_src = up(zi), *c_gid = up(zi), *c_init = up(zu), *c_dummy = up(zu), *c_dis = up(zu), *c_w = up(zd);
            void *c_gpos = up(zg), *c_gvel = up(zg), *c_status = up(zi), *c_best = up(zi), *c_exit = up(zi), *c_cmd = up(zd);
            TMPC_OK_(tmpc_guidance_plan(h, Q, &opt, c_counts, c_classes, explicit_prev ? c_prev : nullptr, c_ids, c_sel, c_mode, c_src, c_init, c_dummy, c_dis, c_gid, c_w), h);
            TMPC_OK_(tmpc_sample_guidance(h, B, R, c_nodes, c_ncount, c_gpos, c_gvel, c_status), h);
            TMPC_OK_(tmpc_guidance_decide(h, Q, &opt, d_pobj, d_code, c_dis, c_gid, c_w, d_state, deceleration, control_dt, enable_output ? 1 : 0, c_best, c_exit, c_cmd, c_ids,
                                          c_sel), h);
            TMPC_OK_(tmpc_synchronize(h), h);
            const bool equal = same(plan.mode, down<int32_t>(c_mode, B)) && same(plan.src, down<int32_t>(c_src, B)) && same(plan.guidance_id, down<int32_t>(c_gid, B)) &&
                               same(plan.init_enabled, down<uint8_t>(c_init, B)) && same(plan.rows_dummy, down<uint8_t>(c_dummy, B)) &&
                               same(plan.disabled, down<uint8_t>(c_dis, B)) && same(plan.weight, down<double>(c_w, B)) && same(gpos, down<double>(c_gpos, gpos.size())) &&
                               same(gvel, down<double>(c_gvel, gvel.size())) && same(status, down<int32_t>(c_status, B)) && same(dec.best, down<int32_t>(c_best, Q)) &&
                               same(dec.exit_code, down<int32_t>(c_exit, Q)) && same(dec.cmd, down<double>(c_cmd, (size_t)Q * 2)) &&
                               same(host_state.planner_ids, down<int32_t>(c_ids, B)) && same(host_state.selection, down<int32_t>(c_sel, (size_t)Q * 3));
            std::printf("equal %d\n", (int)equal);
            for (void *p : {c_nodes, c_ncount, c_counts, c_classes, c_prev, c_mode, c_src, c_gid, c_init, c_dummy, c_dis, c_w, c_gpos, c_gvel, c_status, c_best, c_exit, c_cmd})
                HIP_OK(hipFree(p));
        }
        std::vector<double> v1(B), w0(B);
        for (int b = 0; b < B; b++) { v1[b] = xtraj[(size_t)b * (N + 1) * nx + nx + 3]; w0[b] = utraj[(size_t)b * N * 2 + 1]; }
        line("mode", plan.mode); line("src", plan.src); line("init_enabled", plan.init_enabled); line("rows_dummy", plan.rows_dummy); line("disabled", plan.disabled);
        line("guidance_id", plan.guidance_id); line("weight", plan.weight); line("status", status); line("gpos", gpos); line("gvel", gvel);
        line("pobj", pobj); line("code", code); line("v1", v1); line("w0", w0);
        line("best", dec.best); line("exit", dec.exit_code); line("cmd", dec.cmd); line("ids", host_state.planner_ids); line("sel", host_state.selection);
    }
    if (device) {
        delete twin;
        for (void *p : {d_state, c_ids, c_sel}) HIP_OK(hipFree(p));
        tmpc_destroy(h);
    }
    return 0;
}
