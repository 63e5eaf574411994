// The yardstick of scratch/measure_percolation.py: the serial driver of percolation_plan.h - the rules the kernels run - on one core.
// argv[1]: a file of int64 n[3], int64 connectivity, float64 level, float64 grid[V]; argv[2]: where the labels at `level` go (int32 [V]).
// stdout: one JSON object.  Build: g++ -O2 -std=c++17 -ffp-contract=off -I sitator_amd/csrc.
#include <chrono>
#include <cstdio>
#include <vector>

#include "percolation_plan.h"

static double now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[4];
    double level;
    if (fread(head, 8, 4, f) != 4 || fread(&level, 8, 1, f) != 1) return 2;
    const int64_t *n = head, V = n[0] * n[1] * n[2];
    const int conn = (int)head[3];
    std::vector<double> grid((size_t)V);
    if (fread(grid.data(), 8, (size_t)V, f) != (size_t)V) return 2;
    fclose(f);
    std::vector<int32_t> label((size_t)V), again((size_t)V), rec;
    double t0 = now();
    pc_init_serial(grid.data(), V, level, label.data());
    const int64_t rounds_global = pc_label_serial(n, conn, false, label.data());
    const double t_global = now() - t0;
    t0 = now();
    pc_init_serial(grid.data(), V, level, again.data());
    const int64_t rounds_tile = pc_label_serial(n, conn, true, again.data());
    const double t_tile = now() - t0;
    const bool same = label == again;
    t0 = now();
    pc_seam_serial(n, conn, label.data(), rec);
    const double t_seam = now() - t0;
    PcQuotient q;
    t0 = now();
    const bool ok = pc_quotient(rec.data(), (int64_t)rec.size() / 3, false, q);
    const double t_quotient = now() - t0;
    pc_relabel_serial(V, q.pairs, label.data());
    FILE *out = fopen(argv[2], "wb");
    if (!out || fwrite(label.data(), 4, (size_t)V, out) != (size_t)V) return 2;
    fclose(out);
    double levels[3];
    int32_t ranks[3];
    int64_t passes;
    t0 = now();
    const bool ok_levels = pc_levels_serial(grid.data(), n, conn, false, levels, ranks, &passes);
    const double t_levels = now() - t0;
    printf("{\"ok\": %d, \"labelling_global_seconds\": %.6f, \"rounds_global\": %lld, \"labelling_tile_first_seconds\": %.6f, \"rounds_tile_first\": %lld, "
           "\"forms_equal\": %d, \"seam_seconds\": %.6f, \"seam_records\": %lld, \"distinct_records\": %lld, \"quotient_seconds\": %.6f, "
           "\"max_rank\": %d, \"levels_seconds\": %.6f, \"passes\": %lld, \"levels_hex\": [\"%a\", \"%a\", \"%a\"], \"ranks\": [%d, %d, %d]}\n",
           (int)(ok && ok_levels), t_global, (long long)rounds_global, t_tile, (long long)rounds_tile, (int)same, t_seam, (long long)(rec.size() / 3),
           (long long)q.distinct, t_quotient, q.max_rank, t_levels, (long long)passes, levels[0], levels[1], levels[2], ranks[0], ranks[1], ranks[2]);
    return 0;
}
