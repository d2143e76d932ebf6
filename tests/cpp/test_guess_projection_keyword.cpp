// test_guess_projection_keyword.cpp -- the adapter (ogl_amd/host/OGLAdapter.H over tests/cpp/MiniFoam.H) reads the keyword
// guessProjection from the solver's dictionary and hands it on as the property of the same name: three solver objects on
// one field, as three time steps construct them, find the ring of the field growing; a dictionary without the keyword
// leaves the property at 0; a value outside 0 .. 8 is a fatal error naming the keyword.  Needs the MI355X (the solver's
// constructor opens the device); built and run by tests/test_cpp_guess_projection.py.
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
    dictionary d = cg_dict();
    d.add("guessProjection", 3);
    scalarField psi(c.n, 0.0);
    for (int step = 0; step < 3; ++step) {
        scalarField source(c.n);
        for (label i = 0; i < c.n; ++i) source[i] = std::sin(0.37 * i + 0.1 * step) + 0.25;
        auto solver = lduMatrix::solver::New("p", *c.A, c.bou, c.intc, c.ifaces, d);
        EXPECT_TRUE(property_of(*solver, "guessProjection") == 3.0);
        const solverPerformance perf = solver->solve(psi, source);
        EXPECT_TRUE(perf.finalResidual() < 1e-10);
        EXPECT_TRUE(property_of(*solver, "guessProjectionOffered") == (double)step);
        EXPECT_TRUE(property_of(*solver, "guessProjectionStored") == (double)(step + 1));
        std::printf("step %d: %d iterations, offered %g, kept %g\n", step, (int)perf.nIterations(),
                    property_of(*solver, "guessProjectionOffered"), property_of(*solver, "guessProjectionKept"));
    }
    {   // no keyword: the property is handed on as 0, and a solve publishes nothing of the projection
        scalarField source(c.n, 1.0), x(c.n, 0.0);
        auto solver = lduMatrix::solver::New("q", *c.A, c.bou, c.intc, c.ifaces, cg_dict());
        EXPECT_TRUE(property_of(*solver, "guessProjection") == 0.0);
        solver->solve(x, source);
    }
    for (int bad : {9, -1}) {
        dictionary e = cg_dict();
        e.add("guessProjection", bad);
        std::string msg;
        try {
            lduMatrix::solver::New("r", *c.A, c.bou, c.intc, c.ifaces, e);
        } catch (const Foam::error &err) {
            msg = err.what();
        }
        EXPECT_TRUE(msg.find("guessProjection") != std::string::npos);
    }
    std::printf("%d failure(s)\n", g_failed);
    return g_failed ? 1 : 0;
}
