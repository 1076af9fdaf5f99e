// Linearly transformed cosines fitted on the device (include/vkr_ltc_table.h fit_ltc_table): one wave per chain of texels
// (x, ., i), the samples of an objective evaluation spread over its lanes, the simplex of the minimiser the same in every
// lane.  Binary64 without contraction, like frame_statistics.hip; restated in numpy bit for bit
// (vulkan_renderer_amd/ltc_fit.py).  The comments name the quantities of the header.
#include "vkr_ltc_table.h"
#include "host/vkr_internal.h"
#include <hip/hip_runtime.h>

constexpr double kPi = 3.141592653589793;
constexpr double kInvPi = 1.0 / kPi;
constexpr double kTolerance = 1e-12;

struct fit_args {
	uint32_t resolution, fresnel_count, sample_count, log2_sample_count, max_iterations;
	// sin(theta_y) and cos(theta_y): 2 * resolution doubles; cos and sin of 2 pi t_b: 2 * sample_count doubles
	const double* inclinations;
	const double* azimuths;
	float* fits;
};

__device__ static inline double max_of(double a, double b) { return a > b ? a : b; }

// The sum of the header: the lanes hold the partials, and after the butterfly every lane holds p[0] (IEEE addition commutes).
// The value goes through the first lane so that the compiler knows it to be the same in all of them.
__device__ static inline double wave_sum(double partial) {
#pragma unroll
	for (int h = 32; h != 0; h >>= 1) partial += __shfl_xor(partial, h);
	int low = __builtin_amdgcn_readfirstlane(__double2loint(partial));
	int high = __builtin_amdgcn_readfirstlane(__double2hiint(partial));
	return __hiloint2double(high, low);
}

struct texel {
	double s, c, f0, alpha, a2, g, mk;
	// e, lerp and 1 - lerp of the BRDF set
	double ex, ez, lerp, one_minus_lerp;
	// the stored albedo, the normaliser of the objective, the frame
	double A, An, Zx, Zz;
	bool first;
};

// f(L) and p(L)
__device__ static inline void brdf_and_density(const texel& t, double Lx, double Ly, double Lz, double& f, double& p) {
	double hx = Lx + t.s, hy = Ly, hz = Lz + t.c;
	double r = 1.0 / sqrt((hx * hx + hy * hy) + hz * hz);
	double Hx = hx * r, Hz = hz * r;
	double vh = t.s * Hx + t.c * Hz;
	double q = (Hz * t.a2 - Hz) * Hz + 1.0;
	double ggx = t.a2 / (q * q);
	double masking = Lz * t.g;
	double shadowing = t.c * sqrt((Lz - Lz * t.a2) * Lz + t.a2);
	double smith = 0.5 / (masking + shadowing);
	double ch = vh < 1.0 ? max_of(vh, 0.0) : 1.0;
	double fl = 1.0 - ch;
	double fl2 = fl * fl;
	double fresnel = t.f0 + (1.0 - t.f0) * ((fl2 * fl) * fl2);
	f = Lz > 0.0 ? (((ggx * smith) * fresnel) * kInvPi) * Lz : 0.0;
	p = (t.mk * (ggx * kInvPi)) * 0.25;
}

// The point (cx, cy, cz) of sample k and its weight W
__device__ static inline void grid_point(const fit_args& a, uint32_t k, double& cx, double& cy, double& cz, double& W) {
	uint32_t ia = k >> a.log2_sample_count, ib = k & (a.sample_count - 1);
	double q = 1.0 - ((double) ia + 0.5) / (double) a.sample_count;
	double radius = sqrt(1.0 - q * q);
	cx = radius * a.azimuths[2 * ib];
	cy = radius * a.azimuths[2 * ib + 1];
	cz = q;
	W = 2.0 * q;
}

// Sample (cx, cy) of the BRDF set
__device__ static inline void brdf_sample(const texel& t, double cx, double cy, double& Lx, double& Ly, double& Lz) {
	double sy = sqrt(1.0 - cx * cx) * t.one_minus_lerp + cy * t.lerp;
	double sz = sqrt(max_of(1.0 - (cx * cx + sy * sy), 0.0));
	double nx, ny, nz;
	if (!t.first) { nx = t.ex * sz - t.ez * sy; ny = cx; nz = t.ex * sy + t.ez * sz; }
	else { nx = cx; ny = sy; nz = sz; }
	double mx = t.alpha * nx, my = t.alpha * ny, mz = nz;
	double r = 1.0 / sqrt((mx * mx + my * my) + mz * mz);
	mx *= r; my *= r; mz *= r;
	double two = 2.0 * (mx * t.s + mz * t.c);
	Lx = two * mx - t.s; Ly = two * my; Lz = two * mz - t.c;
}

struct ltc_matrix {
	double M00, M02, M20, M22, m22;
	double i00, i02, i20, i22, i11, idet;
};

// The parameters (m11, m22, m13) of a vertex
__device__ static inline void parameters_of(const texel& t, const double v[3], double out[3]) {
	out[0] = max_of(v[0], 1e-7);
	out[1] = t.first ? out[0] : max_of(v[1], 1e-7);
	out[2] = t.first ? 0.0 : v[2];
}

__device__ static inline ltc_matrix matrix_of(const texel& t, const double v[3]) {
	double m[3];
	parameters_of(t, v, m);
	ltc_matrix M;
	M.M00 = m[0] * t.Zz; M.M02 = m[2] * t.Zz + t.Zx; M.M20 = -(m[0] * t.Zx); M.M22 = t.Zz - m[2] * t.Zx; M.m22 = m[1];
	double det2 = M.M00 * M.M22 - M.M02 * M.M20;
	M.i00 = M.M22 / det2; M.i02 = -M.M02 / det2; M.i20 = -M.M20 / det2; M.i22 = M.M00 / det2;
	M.idet = 1.0 / fabs(M.m22 * det2);
	M.i11 = 1.0 / M.m22;
	return M;
}

// D(L)
__device__ static inline double ltc_density(const ltc_matrix& M, double Lx, double Ly, double Lz) {
	double wx = M.i00 * Lx + M.i02 * Lz, wy = M.i11 * Ly, wz = M.i20 * Lx + M.i22 * Lz;
	double l2 = (wx * wx + wy * wy) + wz * wz;
	return (max_of(wz, 0.0) * M.idet) / (kPi * (l2 * l2));
}

__device__ static inline double term_of(double fa, double p, double D, double Lz, double W) {
	double den = p + D;
	double d = fabs(fa - D);
	return (Lz > 0.0 && den != 0.0) ? (((d * d) * d) / den) * W : 0.0;
}

// E(v)
__device__ static double objective(const fit_args& a, const texel& t, const double v[3], uint32_t lane) {
	ltc_matrix M = matrix_of(t, v);
	double brdf_set = 0.0, ltc_set = 0.0;
	const uint32_t count = a.sample_count << a.log2_sample_count;
	for (uint32_t k = lane; k < count; k += 64) {
		double cx, cy, cz, W, Lx, Ly, Lz, f, p;
		grid_point(a, k, cx, cy, cz, W);
		brdf_sample(t, cx, cy, Lx, Ly, Lz);
		brdf_and_density(t, Lx, Ly, Lz, f, p);
		brdf_set = brdf_set + term_of(f / t.An, p, ltc_density(M, Lx, Ly, Lz), Lz, W);
		Lx = M.M00 * cx + M.M02 * cz; Ly = M.m22 * cy; Lz = M.M20 * cx + M.M22 * cz;
		double r = 1.0 / sqrt((Lx * Lx + Ly * Ly) + Lz * Lz);
		Lx *= r; Ly *= r; Lz *= r;
		brdf_and_density(t, Lx, Ly, Lz, f, p);
		ltc_set = ltc_set + term_of(f / t.An, p, ltc_density(M, Lx, Ly, Lz), Lz, W);
	}
	return (wave_sum(brdf_set) + wave_sum(ltc_set)) / (double) count;
}

// v[k] = q, E[k] = value for the k that is `index` (no indexed registers)
__device__ static inline void store_vertex(double v[4][3], double E[4], uint32_t index, const double q[3], double value) {
#pragma unroll
	for (uint32_t k = 0; k != 4; ++k)
		if (k == index) { v[k][0] = q[0]; v[k][1] = q[1]; v[k][2] = q[2]; E[k] = value; }
}

__device__ static inline void trade_places(double v[4][3], double E[4], int j) {
	if (E[j] < E[j - 1]) {
		double e = E[j]; E[j] = E[j - 1]; E[j - 1] = e;
#pragma unroll
		for (int d = 0; d != 3; ++d) { double x = v[j][d]; v[j][d] = v[j - 1][d]; v[j - 1][d] = x; }
	}
}

// The steps of the minimiser that end in an evaluation of the objective: the loop below has one call of it
enum fit_step { step_first_vertices, step_reflect, step_expand, step_contract_outside, step_contract_inside, step_shrink };

__global__ void __launch_bounds__(64) k_fit_ltc_chains(fit_args a) {
	const uint32_t lane = threadIdx.x;
	const uint32_t R = a.resolution, x = blockIdx.x % R, slice = blockIdx.x / R;
	const uint32_t count = a.sample_count << a.log2_sample_count;
	texel t;
	double ratio = (double) x / (double) (R - 1);
	t.alpha = max_of(ratio * ratio, 0.0064);
	t.a2 = t.alpha * t.alpha;
	t.f0 = (double) slice / (double) (a.fresnel_count - 1);
	double start[3] = {t.alpha, t.alpha, 0.0};
	for (uint32_t y = 0; y != R; ++y) {
		t.first = y == 0;
		t.s = a.inclinations[2 * y]; t.c = a.inclinations[2 * y + 1];
		t.g = sqrt((t.c - t.c * t.a2) * t.c + t.a2);
		t.mk = 2.0 / (t.c + t.g);
		double ex = t.alpha * t.s, ez = t.c;
		double el = sqrt(ex * ex + ez * ez);
		t.ex = ex / el; t.ez = ez / el;
		t.lerp = 0.5 * t.ez + 0.5;
		t.one_minus_lerp = 1.0 - t.lerp;
		// the albedo of the BRDF set; the normaliser and the average direction of both sets under the balance heuristic
		double sum_a = 0.0, sum_w = 0.0, sum_x = 0.0, sum_z = 0.0, sum_cw = 0.0, sum_cx = 0.0, sum_cz = 0.0;
		for (uint32_t k = lane; k < count; k += 64) {
			double cx, cy, cz, W, Lx, Ly, Lz, f, p;
			grid_point(a, k, cx, cy, cz, W);
			brdf_sample(t, cx, cy, Lx, Ly, Lz);
			brdf_and_density(t, Lx, Ly, Lz, f, p);
			sum_a = sum_a + (f / p) * W;
			double wb = (f / (p + max_of(Lz, 0.0) * kInvPi)) * W;
			sum_w = sum_w + wb; sum_x = sum_x + wb * Lx; sum_z = sum_z + wb * Lz;
			brdf_and_density(t, cx, cy, cz, f, p);
			double wc = (f / (p + cz * kInvPi)) * W;
			sum_cw = sum_cw + wc; sum_cx = sum_cx + wc * cx; sum_cz = sum_cz + wc * cz;
		}
		t.A = wave_sum(sum_a) / (double) count;
		t.An = (wave_sum(sum_w) + wave_sum(sum_cw)) / (double) count;
		double ax = (wave_sum(sum_x) + wave_sum(sum_cx)) / (double) count, az = (wave_sum(sum_z) + wave_sum(sum_cz)) / (double) count;
		if (y != 0) {
			double zl = sqrt(ax * ax + az * az);
			t.Zx = ax / zl; t.Zz = az / zl;
		}
		else { t.Zx = 0.0; t.Zz = 1.0; }
		// the second start: the plain cosine lobe, if the objective prefers it
		{
			const double identity[3] = {1.0, 1.0, 0.0};
			if (objective(a, t, identity, lane) < objective(a, t, start, lane)) { start[0] = 1.0; start[1] = 1.0; start[2] = 0.0; }
		}
		// the minimiser: q is the point whose value the step waits for
		double v[4][3], E[4] = {0.0, 0.0, 0.0, 0.0}, q[3] = {start[0], start[1], start[2]}, c[3], r[3], Er = 0.0;
		uint32_t index = 0, iterations = 0;
		fit_step step = step_first_vertices;
		for (;;) {
			double Eq = objective(a, t, q, lane);
			bool shrink = false, ordered = false;
			if (step == step_first_vertices || step == step_shrink) {
				store_vertex(v, E, index, q, Eq);
				++index;
				if (index != 4) {
#pragma unroll
					for (uint32_t k = 1; k != 4; ++k)
						if (k == index) {
#pragma unroll
							for (int d = 0; d != 3; ++d)
								q[d] = step == step_shrink ? v[0][d] + 0.5 * (v[k][d] - v[0][d]) : ((uint32_t) d == k - 1 ? start[d] + 0.05 : start[d]);
						}
					continue;
				}
				ordered = true;
			}
			else if (step == step_reflect) {
				Er = Eq;
#pragma unroll
				for (int d = 0; d != 3; ++d) r[d] = q[d];
				if (Er < E[0]) {
#pragma unroll
					for (int d = 0; d != 3; ++d) q[d] = c[d] + 2.0 * (c[d] - v[3][d]);
					step = step_expand;
					continue;
				}
				else if (Er < E[2]) { store_vertex(v, E, 3, r, Er); ordered = true; }
				else if (Er < E[3]) {
#pragma unroll
					for (int d = 0; d != 3; ++d) q[d] = c[d] + 0.5 * (r[d] - c[d]);
					step = step_contract_outside;
					continue;
				}
				else {
#pragma unroll
					for (int d = 0; d != 3; ++d) q[d] = c[d] + 0.5 * (v[3][d] - c[d]);
					step = step_contract_inside;
					continue;
				}
			}
			else if (step == step_expand) {
				if (Eq < Er) store_vertex(v, E, 3, q, Eq);
				else store_vertex(v, E, 3, r, Er);
				ordered = true;
			}
			else if (step == step_contract_outside) {
				if (Eq <= Er) { store_vertex(v, E, 3, q, Eq); ordered = true; }
				else shrink = true;
			}
			else {
				if (Eq < E[3]) { store_vertex(v, E, 3, q, Eq); ordered = true; }
				else shrink = true;
			}
			if (shrink) {
				index = 1;
#pragma unroll
				for (int d = 0; d != 3; ++d) q[d] = v[0][d] + 0.5 * (v[1][d] - v[0][d]);
				step = step_shrink;
				continue;
			}
			if (ordered) {
				trade_places(v, E, 1);
				trade_places(v, E, 2); trade_places(v, E, 1);
				trade_places(v, E, 3); trade_places(v, E, 2); trade_places(v, E, 1);
				if (iterations == a.max_iterations || E[3] - E[0] < kTolerance) break;
				++iterations;
#pragma unroll
				for (int d = 0; d != 3; ++d) {
					c[d] = ((v[0][d] + v[1][d]) + v[2][d]) / 3.0;
					q[d] = c[d] + (c[d] - v[3][d]);
				}
				step = step_reflect;
			}
		}
		// the fit of the best vertex; the next texel of the chain starts from its parameters
		ltc_matrix M = matrix_of(t, v[0]);
		parameters_of(t, v[0], start);
		if (lane == 0) {
			float* fit = a.fits + 5 * (((size_t) slice * R + y) * R + x);
			fit[0] = (float) (M.M00 / M.M22);
			fit[1] = (float) (M.M20 / M.M22);
			fit[2] = (float) (M.m22 / M.M22);
			fit[3] = (float) (M.M02 / M.M22);
			fit[4] = (float) t.A;
		}
	}
}

extern "C" ltc_fit_settings_t get_default_ltc_fit_settings(void) {
	ltc_fit_settings_t settings = {32, 51, 32, 200};
	return settings;
}

extern "C" void free_ltc_fits(float* fits) {
	free(fits);
}

extern "C" int fit_ltc_table(ltc_table_t* table, float** out_fits, const device_t* device, const ltc_fit_settings_t* settings) {
	memset(table, 0, sizeof(*table));
	if (out_fits) *out_fits = NULL;
	if (!device) {
		printf("fit_ltc_table() needs a device: the fit is a HIP kernel.\n");
		return 1;
	}
	ltc_fit_settings_t s = settings ? *settings : get_default_ltc_fit_settings();
	uint32_t R = s.resolution, F = s.fresnel_count, N = s.sample_count;
	if (R < 2 || R > 256 || F < 2 || F > 256 || N < 8 || N > 128 || (N & (N - 1)) || s.max_iterations == 0) {
		printf("A fitted LTC table needs a resolution and a Fresnel count in 2 ... 256, a sample count that is a power of two in 8 ... 128 and at least one iteration, not %u, %u, %u and %u.\n",
			R, F, N, s.max_iterations);
		return 1;
	}
	size_t fit_count = 5 * (size_t) R * R * F;
	// sin and cos of theta_y, cos and sin of 2 pi t_b, by the C library in binary64
	double* angles = (double*) malloc(sizeof(double) * 2 * ((size_t) R + N));
	float* fits = (float*) malloc(sizeof(float) * fit_count);
	void* device_angles = NULL;
	void* device_fits = NULL;
	if (!angles || !fits) printf("Out of memory for %llu LTC fits.\n", (unsigned long long) (fit_count / 5));
	int failed = !angles || !fits
		|| vkr_device_alloc(&device_angles, device, sizeof(double) * 2 * ((size_t) R + N), "the angles of the LTC fit")
		|| vkr_device_alloc(&device_fits, device, sizeof(float) * fit_count, "the LTC fits");
	if (!failed) {
		for (uint32_t y = 0; y != R; ++y) {
			double theta = (double) y / (double) (R - 1) * (M_PI / 2);
			if (!(theta < 1.57)) theta = 1.57;
			angles[2 * y] = sin(theta);
			angles[2 * y + 1] = cos(theta);
		}
		for (uint32_t b = 0; b != N; ++b) {
			double angle = (2.0 * M_PI) * (((double) b + 0.5) / (double) N);
			angles[2 * R + 2 * b] = cos(angle);
			angles[2 * R + 2 * b + 1] = sin(angle);
		}
		fit_args args;
		args.resolution = R; args.fresnel_count = F; args.sample_count = N; args.max_iterations = s.max_iterations;
		args.log2_sample_count = 0;
		while ((1u << args.log2_sample_count) < N) ++args.log2_sample_count;
		args.inclinations = (const double*) device_angles;
		args.azimuths = args.inclinations + 2 * R;
		args.fits = (float*) device_fits;
		failed = vkr_copy_to_device_async(device_angles, angles, sizeof(double) * 2 * ((size_t) R + N), device);
		if (!failed) {
			k_fit_ltc_chains<<<R * F, 64, 0, (hipStream_t) device->stream>>>(args);
			failed = hip_failed(hipGetLastError(), "fitting the LTC table");
		}
		// (waits for the stream: the upload has read `angles` by then)
		failed = vkr_copy_to_host(fits, device_fits, sizeof(float) * fit_count, device) || failed;
	}
	vkr_device_free(device_angles, device);
	vkr_device_free(device_fits, device);
	free(angles);
	failed = failed || vkr_fill_ltc_table(table, device, fits, R, F);
	if (failed) {
		free(fits);
		memset(table, 0, sizeof(*table));
		return 1;
	}
	if (out_fits) *out_fits = fits;
	else free(fits);
	return 0;
}
