// tests/cpp/ref_sequence.cpp -- one call sequence over the whole fa::SteerableFiltersG2 / G4 surface of the reference, protected
// members included, written so that the SAME source builds against
//   * the reference's own three source files over the stand-in headers of oracle/cvshim (oracle/ref_run.mk -> oracle/_ref/ref_run;
//     its planes are committed as tests/golden/ref_run/), and
//   * the facade, include/cvsteer + libcvsteer.so (cvsteer_amd/facade/Makefile -> tests/cpp/ref_sequence; runs on the GPU).
// It therefore uses nothing but the two classes, a subclass of each that reads the protected m_* members, and of the matrix type
// Mat1f(rows, cols), operator()(row, col), rows and cols.
//
//   ref_sequence <input dir> <output dir>
// reads  image, theta_map, craft_g, craft_h, craft_phase, craft_angle  (<name>.f32: ROWS x COLS raw float32) and writes every plane
// it computes as <name>.f32; tests/golden/ref_run/index.json names them.
#include <cvsteer/SteerableFiltersG2.h>
#include <cvsteer/SteerableFiltersG4.h>

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

namespace {

using fa::Mat1f;

const int ROWS = 24, COLS = 70;
const float THETAS[3] = {0.3f, -1.2f, 1.57079637f};                                        // the last is float(pi / 2)
const int POINTS[7][2] = {{0, 0}, {69, 0}, {0, 23}, {69, 23}, {17, 5}, {40, 11}, {64, 13}};  // (x, y): four corners, three inside
const float PW_PHI[5] = {1.57079637f, 0.0f, 3.14159274f, 0.7f, -2.0f};                     // float(pi / 2), 0, float(pi), ...
const bool PW_SIGNUM[5] = {false, true, true, true, false};

std::string g_in, g_out;

void die(const std::string& what)
{
    std::fprintf(stderr, "ref_sequence: %s\n", what.c_str());
    std::exit(2);
}

Mat1f read_plane(const char* name)
{
    const std::string path = g_in + "/" + name + ".f32";
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) die("cannot read " + path);
    std::vector<float> buf((size_t)ROWS * COLS);
    const size_t got = std::fread(buf.data(), sizeof(float), buf.size(), f);
    std::fclose(f);
    if (got != buf.size()) die("short file " + path);
    Mat1f m(ROWS, COLS);
    for (int r = 0; r < ROWS; ++r)
        for (int c = 0; c < COLS; ++c) m(r, c) = buf[(size_t)r * COLS + c];
    return m;
}

void write_floats(const std::string& name, const std::vector<float>& buf)
{
    const std::string path = g_out + "/" + name + ".f32";
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) die("cannot write " + path);
    const size_t put = std::fwrite(buf.data(), sizeof(float), buf.size(), f);
    if (std::fclose(f) != 0 || put != buf.size()) die("short write " + path);
}

void write_plane(const std::string& name, const Mat1f& m)
{
    if (m.rows != ROWS || m.cols != COLS) die(name + ": not a ROWS x COLS plane");
    std::vector<float> buf((size_t)ROWS * COLS);
    for (int r = 0; r < ROWS; ++r)
        for (int c = 0; c < COLS; ++c) buf[(size_t)r * COLS + c] = m(r, c);
    write_floats(name, buf);
}

// the protected members are filled by setup(); the second setup() in the constructor body runs on an object that already IS the
// subclass (the facade copies its GPU state into the members only for subclass objects; the reference simply filters again)
class ProbeG2 : public fa::SteerableFiltersG2 {
public:
    ProbeG2(const Mat1f& image, int width, float spacing) : fa::SteerableFiltersG2(image, width, spacing) { setup(image); }
    const Mat1f& basis(int i) const
    {
        const Mat1f* all[7] = {&m_g2a, &m_g2b, &m_g2c, &m_h2a, &m_h2b, &m_h2c, &m_h2d};
        return *all[i];
    }
    const Mat1f& c1() const { return m_c1; }
    const Mat1f& c2() const { return m_c2; }
    const Mat1f& c3() const { return m_c3; }
    static void callWrap(const Mat1f& angle, Mat1f& out) { wrap(angle, out); }
};

class ProbeG4 : public fa::SteerableFiltersG4 {
public:
    ProbeG4(const Mat1f& image, int width, float spacing) : fa::SteerableFiltersG4(image, width, spacing) { setup(image); }
    const Mat1f& basis(int i) const
    {
        const Mat1f* all[11] = {&m_g4a, &m_g4b, &m_g4c, &m_g4d, &m_g4e, &m_h4a, &m_h4b, &m_h4c, &m_h4d, &m_h4e, &m_h4f};
        return *all[i];
    }
};

std::string num(const std::string& stem, int i)
{
    char b[16];
    std::snprintf(b, sizeof b, "%d", i);
    return stem + b;
}

// steer(theta, ...) in its two-output and its five-output form, for a scalar or a plane of angles
template <class Theta>
void steer_both(ProbeG2& f, const Theta& theta, const std::string& stem)
{
    Mat1f g, h, g5, h5, e, mag, phase;
    f.steer(theta, g, h);
    f.steer(theta, g5, h5, e, mag, phase);
    write_plane(stem + "_g", g);
    write_plane(stem + "_h", h);
    write_plane(stem + "_g5", g5);
    write_plane(stem + "_h5", h5);
    write_plane(stem + "_e", e);
    write_plane(stem + "_mag", mag);
    write_plane(stem + "_phase", phase);
}

void run()
{
    const Mat1f image = read_plane("image"), theta_map = read_plane("theta_map");
    const Mat1f craft_g = read_plane("craft_g"), craft_h = read_plane("craft_h");
    const Mat1f craft_phase = read_plane("craft_phase"), craft_angle = read_plane("craft_angle");

    // ---- G2 at the default (4, 0.67) ----
    ProbeG2 f(image, 4, 0.67f);
    for (int i = 0; i < 7; ++i) write_plane(num("g2_basis_", i), f.basis(i));
    write_plane("g2_c1", f.c1());
    write_plane("g2_c2", f.c2());
    write_plane("g2_c3", f.c3());
    const Mat1f& dominant = f.getDominantOrientationAngle();
    write_plane("g2_theta", dominant);
    write_plane("g2_strength", f.getDominantOrientationStrength());
    for (int k = 0; k < 3; ++k) steer_both(f, THETAS[k], num("g2_s", k));
    steer_both(f, dominant, "g2_dom");
    steer_both(f, theta_map, "g2_map");
    {
        std::vector<float> pts;   // [theta][point][g, h, g, h, e, magnitude, phase]
        for (int k = 0; k < 3; ++k)
            for (int p = 0; p < 7; ++p) {
                const fa::Point at(POINTS[p][0], POINTS[p][1]);
                float v[7] = {0, 0, 0, 0, 0, 0, 0};
                f.steer(at, THETAS[k], v[0], v[1]);
                f.steer(at, THETAS[k], v[2], v[3], v[4], v[5], v[6]);
                pts.insert(pts.end(), v, v + 7);
            }
        write_floats("g2_points", pts);
    }
    {
        Mat1f g, h, e, mag, phase, out;   // the callers' sequence: the three maps on its own magnitude and phase
        f.steer(dominant, g, h, e, mag, phase);
        f.findEdges(mag, phase, out);
        write_plane("g2_find_edges", out);
        Mat1f dark, bright;
        f.findDarkLines(mag, phase, dark);
        write_plane("g2_find_dark", dark);
        f.findBrightLines(mag, phase, bright);
        write_plane("g2_find_bright", bright);
    }

    // ---- crafted per-pixel inputs through the entries that take planes ----
    {
        Mat1f mag, phase, wrapped;
        f.computeMagnitudeAndPhase(craft_g, craft_h, mag, phase);
        write_plane("craft_mag", mag);
        write_plane("craft_phase_out", phase);
        ProbeG2::callWrap(craft_angle, wrapped);
        write_plane("craft_wrap", wrapped);
        for (int k = 0; k < 5; ++k) {
            Mat1f lambda;
            fa::SteerableFiltersG2::phaseWeights(craft_phase, lambda, PW_PHI[k], PW_SIGNUM[k], 2.0f);
            write_plane(num("craft_pw", k), lambda);
        }
        Mat1f ones(ROWS, COLS), edges, dark, bright;
        for (int r = 0; r < ROWS; ++r)
            for (int c = 0; c < COLS; ++c) ones(r, c) = 1.0f;
        f.findEdges(ones, craft_phase, edges);
        f.findDarkLines(ones, craft_phase, dark);
        f.findBrightLines(ones, craft_phase, bright);
        write_plane("craft_edges", edges);
        write_plane("craft_dark", dark);
        write_plane("craft_bright", bright);
    }

    // ---- G4 at the default (6, 0.5) ----
    {
        ProbeG4 f4(image, 6, 0.5f);
        for (int i = 0; i < 11; ++i) write_plane(num("g4_basis_", i), f4.basis(i));
        Mat1f g, h;
        f4.steer(0.3f, g, h);
        write_plane("g4_s0_g", g);
        write_plane("g4_s0_h", h);
        Mat1f g1, h1;
        f4.steer(-2.0f, g1, h1);
        write_plane("g4_s1_g", g1);
        write_plane("g4_s1_h", h1);
        Mat1f gm, hm;
        f4.steer(theta_map, gm, hm);
        write_plane("g4_map_g", gm);
        write_plane("g4_map_h", hm);
    }

    // ---- widths no kernel is specialised for ----
    {
        ProbeG2 f2(image, 3, 0.9f);
        for (int i = 0; i < 7; ++i) write_plane(num("g2w3_basis_", i), f2.basis(i));
        Mat1f g, h;
        f2.steer(0.3f, g, h);
        write_plane("g2w3_g", g);
        write_plane("g2w3_h", h);
        ProbeG4 f4(image, 4, 0.75f);
        for (int i = 0; i < 11; ++i) write_plane(num("g4w4_basis_", i), f4.basis(i));
        Mat1f g4, h4;
        f4.steer(0.3f, g4, h4);
        write_plane("g4w4_g", g4);
        write_plane("g4w4_h", h4);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) die("usage: ref_sequence <input dir> <output dir>");
    g_in = argv[1];
    g_out = argv[2];
    try {
        run();
    } catch (const std::exception& ex) {
        die(ex.what());
    }
    std::printf("ref_sequence OK\n");
    return 0;
}
