// tests/cpp/test_episode.cpp -- MPCPlanner::episodeStep (mpc_planner/episode.h) on a case file of tests/test_cpp_episode.py: every array after
// every tick, %.17g (a double round-trips), for the comparison with mpc_planner_amd/modules.py episode_step.  Host code only, no GPU.
//   test_episode <case.bin>
// The file is a flat array of doubles: Q R P nx ticks substeps timeout_ticks max_episodes control_dt max_acceleration max_angular_velocity
// robot_radius goal_x has_box has_goal, plant0 [Q][6], count [Q], raw_pos0 [Q][R][2], raw_vel0 [Q][R][2], raw_radius [Q][R], box [Q][4] if
// has_box, goal [Q][3] if has_goal, commands [ticks][Q][2].  The in/out arrays start at the start arrays / zeros, the outputs sentinel-filled.
#include <cstdint>
#include <cstdio>
#include <vector>

#include <mpc_planner/episode.h>

template <class T> static void print(const char *name, const std::vector<T> &v)
{
    std::printf("%s", name);
    for (const T &x : v) std::printf(" %.17g", (double)x);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> in;
    double buf[256];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
    size_t at = 0;
    auto take = [&](size_t n) { std::vector<double> v(in.begin() + at, in.begin() + at + n); at += n; return v; };
    if (in.size() < 15) return 2;
    const std::vector<double> head = take(15);
    const int Q = (int)head[0], R = (int)head[1], P = (int)head[2], nx = (int)head[3], ticks = (int)head[4];
    MPCPlanner::EpisodeOptions o;
    o.substeps = (int)head[5]; o.timeout_ticks = (int)head[6]; o.max_episodes = (int)head[7]; o.control_dt = head[8]; o.max_acceleration = head[9];
    o.max_angular_velocity = head[10]; o.robot_radius = head[11]; o.goal_x = head[12];
    const bool has_box = head[13] != 0., has_goal = head[14] != 0.;
    if (Q <= 0 || R < 0 || P < 1 || nx < 4 || ticks < 0 || o.max_episodes < 1) return 2;
    const size_t need = 15 + (size_t)Q * (6 + 1 + 5 * (size_t)R + (has_box ? 4 : 0) + (has_goal ? 3 : 0) + 2 * (size_t)ticks);
    if (in.size() != need) return 2;
    const std::vector<double> plant0 = take((size_t)Q * 6), countd = take(Q), raw_pos0 = take((size_t)Q * R * 2), raw_vel0 = take((size_t)Q * R * 2),
                              raw_radius = take((size_t)Q * R), box = take(has_box ? (size_t)Q * 4 : 0), goal = take(has_goal ? (size_t)Q * 3 : 0);
    std::vector<int32_t> count(countd.begin(), countd.end());
    std::vector<double> plant = plant0, raw_pos = raw_pos0, raw_vel = raw_vel0, episode_f((size_t)Q * 2, 0.), log((size_t)Q * o.max_episodes * 4, -3.),
                        state4((size_t)Q * 4, -3.), state_nx((size_t)Q * nx, -3.), state_batch((size_t)Q * P * nx, -3.);
    std::vector<int32_t> episode((size_t)Q * 4, 0), planner_ids((size_t)Q * P, -7), selection((size_t)Q * 3, -7), segment(Q, -7);
    std::vector<uint8_t> was_reset(Q, 9);
    for (int t = 0; t < ticks; t++) {
        const std::vector<double> cmd = take((size_t)Q * 2);
        if (!MPCPlanner::episodeStep(Q, R, P, nx, o, cmd.data(), plant.data(), plant0.data(), count.data(), raw_pos.data(), raw_vel.data(), raw_radius.data(),
                                     raw_pos0.data(), raw_vel0.data(), has_box ? box.data() : nullptr, has_goal ? goal.data() : nullptr, episode.data(),
                                     episode_f.data(), log.data(), was_reset.data(), state4.data(), state_nx.data(), state_batch.data(),
                                     planner_ids.data(), selection.data(), segment.data())) {
            std::printf("refused\n");
            return 3;
        }
        std::printf("tick %d\n", t);
        print("plant", plant); print("raw_pos", raw_pos); print("raw_vel", raw_vel); print("episode", episode); print("episode_f", episode_f);
        print("log", log); print("was_reset", was_reset); print("state4", state4); print("state_nx", state_nx); print("state_batch", state_batch);
        print("planner_ids", planner_ids); print("selection", selection); print("segment", segment);
    }
    return 0;
}
