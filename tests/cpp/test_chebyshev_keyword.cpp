// test_chebyshev_keyword.cpp -- the adapter (ogl_amd/host/OGLAdapter.H over tests/cpp/MiniFoam.H) knows the word Chebyshev,
// reads chebyshevDegree, chebyshevEigRatio and chebyshevLambdaMax from the preconditioner sub-dictionary and hands them on
// as the properties of the same names: a solve runs on what the keywords ask for, a dictionary without them hands on the
// defaults 4 / 30 / 0, a degree outside 1 .. 16 is a fatal error naming the keyword, and so is an unknown preconditioner
// word.  Needs the MI355X (the solver's constructor opens the device); built and run by tests/test_cpp_chebyshev.py.
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

static dictionary cg_dict(const dictionary &pc)
{
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
    scalarField source(c.n);
    for (label i = 0; i < c.n; ++i) source[i] = std::sin(0.37 * i) + 0.25;
    int iterations[3] = {0, 0, 0};
    for (int with = 0; with < 3; ++with) {  // BJ(1) | Chebyshev with its defaults | with the three keywords
        dictionary pc;
        pc.add("preconditioner", with ? "Chebyshev" : "BJ");
        if (with == 2) pc.add("chebyshevDegree", 2).add("chebyshevEigRatio", 12.5).add("chebyshevLambdaMax", 1.875);
        const dictionary d = cg_dict(pc);  // (the solver keeps a reference to its dictionary, as OpenFOAM's does)
        const word field = with == 0 ? "p_bj" : (with == 1 ? "p_default" : "p_keywords");
        scalarField psi(c.n, 0.0);
        auto solver = lduMatrix::solver::New(field, *c.A, c.bou, c.intc, c.ifaces, d);
        const solverPerformance perf = solver->solve(psi, source);
        EXPECT_TRUE(perf.finalResidual() <= 1e-10);
        iterations[with] = (int)perf.nIterations();
        if (with) {
            EXPECT_TRUE(property_of(*solver, "chebyshevDegree") == (with == 2 ? 2.0 : 4.0));
            EXPECT_TRUE(property_of(*solver, "chebyshevEigRatio") == (with == 2 ? 12.5 : 30.0));
            EXPECT_TRUE(property_of(*solver, "chebyshevLambdaMax") == (with == 2 ? 1.875 : 0.0));
            EXPECT_TRUE(property_of(*solver, "chebyshevLaunchesPerApply") == (with == 2 ? 3.0 : 5.0));
            EXPECT_TRUE(property_of(*solver, "chebyshevFusedInUse") == 1.0);
            if (with == 2) {
                EXPECT_TRUE(property_of(*solver, "chebyshevLambdaMaxInUse") == 1.875);
                EXPECT_TRUE(property_of(*solver, "chebyshevLambdaMinInUse") == 1.875 / 12.5);
            } else {
                const double lmax = property_of(*solver, "chebyshevLambdaMaxInUse");
                EXPECT_TRUE(lmax > 1.0 && lmax < 2.0);  // (the Gershgorin bound of a diagonally dominant D^-1 A)
            }
        }
        std::printf("%s: %d iterations, final residual %.3e\n", field.c_str(), iterations[with], (double)perf.finalResidual());
    }
    EXPECT_TRUE(iterations[1] > 0 && 2 * iterations[1] < iterations[0]);
    for (const int degree : {0, 17}) {
        dictionary pc;
        pc.add("preconditioner", "Chebyshev").add("chebyshevDegree", degree);
        const dictionary d = cg_dict(pc);
        std::string msg;
        try {
            lduMatrix::solver::New(degree ? "bad_high" : "bad_low", *c.A, c.bou, c.intc, c.ifaces, d);
        } catch (const Foam::error &err) {
            msg = err.what();
        }
        EXPECT_TRUE(msg.find("chebyshevDegree") != std::string::npos);
    }
    {
        dictionary pc;
        pc.add("preconditioner", "Tschebyscheff");
        const dictionary d = cg_dict(pc);
        std::string msg;
        try {
            lduMatrix::solver::New("bad_word", *c.A, c.bou, c.intc, c.ifaces, d);
        } catch (const Foam::error &err) {
            msg = err.what();
        }
        EXPECT_TRUE(msg.find("Tschebyscheff") != std::string::npos && msg.find("Chebyshev") != std::string::npos);
    }
    std::printf("%d failure(s)\n", g_failed);
    return g_failed ? 1 : 0;
}
