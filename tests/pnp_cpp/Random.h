// Test-owned stand-in for DBoW2's DUtils/Random.h: RandomInt from a seeded generator that logs every call (its range and its answer).
#ifndef DUTILS_RANDOM_H
#define DUTILS_RANDOM_H
#include <vector>
namespace DUtils
{
class Random
{
public:
    struct Call { int min, max, value; };
    static std::vector<Call>& Log() { static std::vector<Call> log; return log; }
    static unsigned long long& State() { static unsigned long long s = 0x2545F4914F6CDD1Dull; return s; }
    static void SeedRand(int seed) { State() = 0x2545F4914F6CDD1Dull ^ ((unsigned long long)seed * 0x9E3779B97F4A7C15ull); }
    static int RandomInt(int min, int max)
    {
        unsigned long long& s = State();
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const int v = min + (int)((s >> 33) % (unsigned long long)(max - min + 1));
        const Call c = {min, max, v};
        Log().push_back(c);
        return v;
    }
};
}
#endif
