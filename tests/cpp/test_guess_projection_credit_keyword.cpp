// test_guess_projection_credit_keyword.cpp -- the adapter (ogl_amd/host/OGLAdapter.H over tests/cpp/MiniFoam.H) reads the
// Switch guessProjectionCredit and the word guessProjectionProducts from the solver's dictionary and hands them on as
// the properties of the same names: three solver
// objects on one field under a relTol, as three time steps construct them, find the credit applied from the second solve
// on (the first has nothing to project on); a dictionary without the keyword hands on 0 and nothing is credited; a value
// that is no Switch is a fatal error naming the keyword.  Needs the MI355X (the solver's constructor opens the device);
// built and run by tests/test_cpp_guess_projection_credit.py.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "MiniFoam.H"
#include "OGLAdapter.H"

OGL_REGISTER_SOLVERS

using namespace Foam;

static int g_failed = 0;
#define EXPECT_TRUE(c)                                                         \
    do {                                                                       \
        if (!(c)) {                                                            \
            std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            ++g_failed;                                                        \
        }                                                                      \
    } while (0)

struct Case {
    objectRegistry db;
    lduMesh mesh{db};
    std::unique_ptr<lduAddressing> addr;
    std::unique_ptr<lduMatrix> A;
    FieldField<Field, scalar> bou, intc;
    lduInterfaceFieldPtrsList ifaces;
    label n = 0;
};

static void build_poisson(Case &c, int nx, int ny, int nz)
{
    std::vector<label> lo, up;
    const label N = nx * ny * nz;
    std::vector<scalar> diag(N);
    for (label cell = 0; cell < N; ++cell) {
        const int i = cell % nx, j = (cell / nx) % ny, k = cell / (nx * ny);
        const int nb = (i > 0) + (i < nx - 1) + (j > 0) + (j < ny - 1) + (k > 0) + (k < nz - 1);
        diag[cell] = nb + 1e-3 * (1.0 + (cell % 7) / 7.0);
        if (i < nx - 1) { lo.push_back(cell); up.push_back(cell + 1); }
        if (j < ny - 1) { lo.push_back(cell); up.push_back(cell + nx); }
        if (k < nz - 1) { lo.push_back(cell); up.push_back(cell + nx * ny); }
    }
    c.n = N;
    c.addr = std::make_unique<lduAddressing>(labelList(lo), labelList(up));
    c.A = std::make_unique<lduMatrix>(c.mesh, *c.addr, scalarField(diag), scalarField(static_cast<label>(lo.size()), -1.0));
}

static dictionary cg_dict()
{
    dictionary pc;
    pc.add("preconditioner", "BJ").add("maxBlockSize", 1);
    dictionary d;
    d.add("solver", "GKOCG").add("preconditioner", pc).add("tolerance", 1e-10).add("relTol", 0.0);
    d.add("maxIter", 300).add("matrixFormat", "Csr").add("executor", "hip").add("adaptMinIter", "false");
    d.add("updateInitGuess", "true");
    return d;
}

static double property_of(const lduMatrix::solver &s, const char *key)
{
    return dynamic_cast<const GKOlduBaseSolver &>(s).backend_property(key);
}

int main()
{
    Case c;
    build_poisson(c, 10, 9, 7);
    for (const char *credit : {"on", "absent", "off"}) {
        dictionary d = cg_dict();
        d.add("relTol", 0.05);
        d.add("guessProjection", 3);
        const bool on = std::string(credit) == "on";
        if (std::string(credit) != "absent") d.add("guessProjectionCredit", credit);
        if (on) d.add("guessProjectionProducts", "onePass");
        scalarField psi(c.n, 0.0);
        const word field = std::string("p_") + credit;
        for (int step = 0; step < 3; ++step) {
            scalarField source(c.n);
            for (label i = 0; i < c.n; ++i) source[i] = std::sin(0.37 * i + 0.1 * step) + 0.25;
            auto solver = lduMatrix::solver::New(field, *c.A, c.bou, c.intc, c.ifaces, d);
            EXPECT_TRUE(property_of(*solver, "guessProjectionCredit") == (on ? 1.0 : 0.0));
            EXPECT_TRUE(property_of(*solver, "guessProjectionProducts") == (on ? 1.0 : 0.0));
            const solverPerformance perf = solver->solve(psi, source);
            const double kept = property_of(*solver, "guessProjectionKept");
            EXPECT_TRUE(property_of(*solver, "guessProjectionOffered") == (double)step);
            EXPECT_TRUE(step == 0 || kept >= 1.0);
            EXPECT_TRUE(property_of(*solver, "guessProjectionCreditInUse") == (on && step > 0 ? 1.0 : 0.0));
            std::printf("credit %s, step %d: %d iterations, initial residual %.3e, kept %g\n", credit, step,
                        (int)perf.nIterations(), (double)perf.initialResidual(), kept);
        }
    }
    {
        dictionary e = cg_dict();
        e.add("guessProjection", 3).add("guessProjectionCredit", "perhaps");
        std::string msg;
        try {
            lduMatrix::solver::New("r", *c.A, c.bou, c.intc, c.ifaces, e);
        } catch (const Foam::error &err) {
            msg = err.what();
        }
        EXPECT_TRUE(msg.find("guessProjectionCredit") != std::string::npos);
    }
    {
        dictionary e = cg_dict();
        e.add("guessProjection", 3).add("guessProjectionProducts", "both");
        std::string msg;
        try {
            lduMatrix::solver::New("r2", *c.A, c.bou, c.intc, c.ifaces, e);
        } catch (const Foam::error &err) {
            msg = err.what();
        }
        EXPECT_TRUE(msg.find("guessProjectionProducts") != std::string::npos);
    }
    std::printf("%d failure(s)\n", g_failed);
    return g_failed ? 1 : 0;
}
