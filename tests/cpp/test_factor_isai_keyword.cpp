// test_factor_isai_keyword.cpp -- the adapter (ogl_amd/host/OGLAdapter.H over tests/cpp/MiniFoam.H) reads the word
// triangularSolves and the label factorSweeps from the preconditioner sub-dictionary and hands them on as the properties of
// the same names: a solve with IC runs on what the keywords ask for, a dictionary without them hands on 0 / 0, and a word
// that is neither exact nor isai (a label outside 0 .. 10) is a fatal error naming the keyword.  Needs the MI355X (the
// solver's constructor opens the device); built and run by tests/test_cpp_factor_isai.py.
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
    int iterations[2] = {0, 0};
    for (int with = 0; with < 2; ++with) {
        dictionary pc;
        pc.add("preconditioner", "IC");
        if (with) pc.add("triangularSolves", "isai").add("factorSweeps", 3).add("sparsityPower", 2);
        const dictionary d = cg_dict(pc);  // (the solver keeps a reference to its dictionary, as OpenFOAM's does)
        const word field = with ? "p_isai" : "p_exact";
        scalarField psi(c.n, 0.0);
        auto solver = lduMatrix::solver::New(field, *c.A, c.bou, c.intc, c.ifaces, d);
        EXPECT_TRUE(property_of(*solver, "triangularSolves") == (with ? 1.0 : 0.0));
        EXPECT_TRUE(property_of(*solver, "factorSweeps") == (with ? 3.0 : 0.0));
        const solverPerformance perf = solver->solve(psi, source);
        EXPECT_TRUE(property_of(*solver, "triangularSolvesInUse") == (with ? 1.0 : 0.0));
        EXPECT_TRUE(property_of(*solver, "factorSweepsInUse") == (with ? 3.0 : 0.0));
        EXPECT_TRUE(property_of(*solver, "iluLaunchesPerApply") == 2.0 || !with);
        EXPECT_TRUE(perf.finalResidual() <= 1e-10);
        iterations[with] = (int)perf.nIterations();
        std::printf("IC %s: %d iterations, final residual %.3e\n", with ? "isai, 3 sweeps, p = 2" : "exact",
                    iterations[with], (double)perf.finalResidual());
    }
    EXPECT_TRUE(iterations[0] > 0 && iterations[1] >= iterations[0]);  // (the approximate inverse is no better than the solve)
    const std::pair<const char *, const char *> bad[] = {{"triangularSolves", "jacobi"}, {"factorSweeps", "11"}};
    for (const auto &kv : bad) {
        dictionary pc;
        pc.add("preconditioner", "IC");
        if (std::string(kv.first) == "factorSweeps") pc.add(kv.first, 11);
        else pc.add(kv.first, kv.second);
        const dictionary d = cg_dict(pc);
        const word field = std::string("bad_") + kv.first;
        std::string msg;
        try {
            lduMatrix::solver::New(field, *c.A, c.bou, c.intc, c.ifaces, d);
        } catch (const Foam::error &err) {
            msg = err.what();
        }
        EXPECT_TRUE(msg.find(kv.first) != std::string::npos);
    }
    std::printf("%d failure(s)\n", g_failed);
    return g_failed ? 1 : 0;
}
