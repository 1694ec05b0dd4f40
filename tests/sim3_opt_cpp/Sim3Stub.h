// Test-owned stand-in for the Sim3 type of the reference's signature: the accessors OptimizeSim3Device uses and nothing else - rotation().coeffs()
// (x, y, z, w), translation(), scale().  It counts the non-const accesses, so a test can tell whether the drop-in wrote to it.
#ifndef SIM3STUB_H
#define SIM3STUB_H
struct StubQuaternion
{
    double v[4];
    double* coeffs() { return v; }
    const double* coeffs() const { return v; }
};
struct StubVector3
{
    double v[3];
    double& operator[](int i) { return v[i]; }
    const double& operator[](int i) const { return v[i]; }
};
struct StubSim3
{
    StubQuaternion r; StubVector3 t; double s; int writes;
    StubSim3() : s(1.0), writes(0) { r.v[0] = r.v[1] = r.v[2] = 0.0; r.v[3] = 1.0; t.v[0] = t.v[1] = t.v[2] = 0.0; }
    const StubQuaternion& rotation() const { return r; }
    StubQuaternion& rotation() { writes++; return r; }
    const StubVector3& translation() const { return t; }
    StubVector3& translation() { writes++; return t; }
    const double& scale() const { return s; }
    double& scale() { writes++; return s; }
};
#endif
