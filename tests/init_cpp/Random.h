// Test-owned stand-in for DBoW2's DUtils/Random.h with the generator the reference uses: the C library's rand(), seeded once per process by
// SeedRandOnce, scaled to the range as rand() / (RAND_MAX + 1) in double.  tests/init_model.py (draw_sets with libc_rand) restates the same.
#ifndef DUTILS_RANDOM_H
#define DUTILS_RANDOM_H
#include <cstdlib>
namespace DUtils
{
class Random
{
public:
    static bool& Seeded() { static bool seeded = false; return seeded; }
    static long& Calls() { static long calls = 0; return calls; }
    static void SeedRandOnce(int seed) { if (!Seeded()) { srand(seed); Seeded() = true; } }
    static int RandomInt(int min, int max)
    {
        Calls()++;
        const int d = max - min + 1;
        return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
    }
};
}
#endif
