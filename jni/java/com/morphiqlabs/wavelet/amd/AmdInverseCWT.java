package com.morphiqlabs.wavelet.amd;

import com.morphiqlabs.wavelet.api.ContinuousWavelet;
import com.morphiqlabs.wavelet.cwt.CWTResult;
import com.morphiqlabs.wavelet.cwt.InverseCWT;

/**
 * MI355X drop-in for {@code InverseCWT.reconstruct} / {@code reconstructBand} / {@code reconstructFrequencyBand}
 * (cwt/InverseCWT.java), for one result or a batch of results over the same scales in one engine call, over the
 * {@code icwtAoS} native (include/vectorwave_amd.h vw_icwt_f64).
 *
 * <p>The real plane of a result is read ({@code getCoefficients()}), complex wavelets included, and the route is the
 * reference's (:213):
 * <ul>
 * <li>{@code n >= 128} (reconstructInternalRealFFT :225-270): the weighted sum of circular convolutions over
 * {@code M = nextPowerOfTwo(n)} that the reference's FFTs evaluate,
 * {@code r[i] = (sum_s wt_s sum_d g_s(d) z_s[(i - d) mod M]) / C_psi}, {@code g_s(d) = psi(d / a_s) / sqrt(a_s)} for
 * {@code d} in {@code (-M/2, M/2]} (createWaveletFFT :561-586), {@code wt_s = weights[s] / a_s}.  A table is cut at
 * its outermost non-zero entries.  The engine evaluates the sum in a fixed order, so the result differs from the
 * reference's by its FFT's rounding (about 1e-15).</li>
 * <li>{@code n < 128} (reconstructInternalRealDirect :275-314): the reference's loops term by term,
 * {@code sum += coeff * kernelValue * weight / scale} with coefficients under 1e-10 skipped; the table holds
 * {@code (1.0 / sqrt(a)) * psi((t - b) / a)}.  The result is the reference's bit for bit.</li>
 * </ul>
 * The tables are built with the wavelet's own {@code psi}; the admissibility constant is the reference's
 * ({@code new InverseCWT(wavelet).getAdmissibilityConstant()}), and so are validation and messages.
 *
 * <p>Not here: MODWTBasedInverseCWT, reconstruction from complex coefficients (the reference has none).
 *
 * <p>Not built or run in this repository (no JDK in its build image): INTEGRATION.md section 2.
 */
public final class AmdInverseCWT {
    private final ContinuousWavelet wavelet;
    private final double admissibilityConstant;

    public AmdInverseCWT(ContinuousWavelet wavelet) {
        // the reference's constructor validates the wavelet and computes C_psi (:62-77)
        this.admissibilityConstant = new InverseCWT(wavelet).getAdmissibilityConstant();
        this.wavelet = wavelet;
    }

    public double getAdmissibilityConstant() {
        return admissibilityConstant;
    }

    public boolean isAdmissible() {
        return admissibilityConstant > 0 && admissibilityConstant < Double.POSITIVE_INFINITY;
    }

    /** {@code InverseCWT.reconstruct(cwtResult)} (:94-116). */
    public double[] reconstruct(CWTResult cwtResult) {
        if (cwtResult == null) throw new IllegalArgumentException("CWT result cannot be null");
        return reconstruct(new CWTResult[] {cwtResult})[0];
    }

    /** {@code reconstruct(results[b])} for every result (all over the same scales and length), one engine call. */
    public double[][] reconstruct(CWTResult[] results) {
        final double[] scales = checked(results);
        return run(results, scales, 0, scales.length);
    }

    /** {@code InverseCWT.reconstructBand(cwtResult, minScale, maxScale)} (:132-171). */
    public double[] reconstructBand(CWTResult cwtResult, double minScale, double maxScale) {
        if (cwtResult == null) throw new IllegalArgumentException("CWT result cannot be null");
        return reconstructBand(new CWTResult[] {cwtResult}, minScale, maxScale)[0];
    }

    public double[][] reconstructBand(CWTResult[] results, double minScale, double maxScale) {
        if (results == null || results.length == 0 || results[0] == null) {
            throw new IllegalArgumentException("CWT result cannot be null");
        }
        if (minScale <= 0 || maxScale <= minScale) {
            throw new IllegalArgumentException("Invalid scale range: minScale=" + minScale + ", maxScale=" + maxScale);
        }
        final double[] scales = results[0].getScales();
        int startIdx = -1, endIdx = -1;
        for (int i = 0; i < scales.length; i++) {
            if (startIdx == -1 && scales[i] >= minScale) startIdx = i;
            if (scales[i] > maxScale) {
                endIdx = i;
                break;
            }
        }
        if (startIdx == -1) startIdx = 0;
        if (endIdx == -1) endIdx = scales.length;
        if (startIdx >= endIdx) return new double[results.length][results[0].getNumSamples()];   // :164-167
        return run(results, scales, startIdx, endIdx);
    }

    /** {@code InverseCWT.reconstructFrequencyBand} (:187-205). */
    public double[] reconstructFrequencyBand(CWTResult cwtResult, double samplingRate, double minFreq, double maxFreq) {
        if (samplingRate <= 0) throw new IllegalArgumentException("Sampling rate must be positive");
        if (minFreq < 0 || maxFreq <= minFreq || maxFreq > samplingRate / 2) {
            throw new IllegalArgumentException("Invalid frequency range: minFreq=" + minFreq + ", maxFreq=" + maxFreq);
        }
        final double centerFreq = wavelet.centerFrequency();
        return reconstructBand(cwtResult, centerFreq * samplingRate / maxFreq, centerFreq * samplingRate / minFreq);
    }

    private static double[] checked(CWTResult[] results) {
        if (results == null || results.length == 0 || results[0] == null) {
            throw new IllegalArgumentException("CWT result cannot be null");
        }
        final double[] scales = results[0].getScales();
        if (scales == null || scales.length == 0) throw new IllegalArgumentException("CWT result has no scales");
        final int n = results[0].getNumSamples();
        if (n <= 0) throw new IllegalArgumentException("Invalid signal length: " + n);
        final double[][] coeffs = results[0].getCoefficients();
        if (coeffs == null || coeffs.length == 0) throw new IllegalArgumentException("CWT result has no coefficients");
        return scales;
    }

    private double[][] run(CWTResult[] results, double[] scales, int start, int end) {
        final int batch = results.length, n = results[0].getNumSamples(), numPlanes = scales.length;
        final int count = end - start;
        final double[] weights = logScaleWeights(scales, start, end);
        final boolean sum = n >= 128;   // :213
        final int m = nextPowerOfTwo(n);

        long[] desc = new long[4 * count];
        double[] wts = new double[2 * count];
        double[][] tables = new double[count][];
        int total = 0;
        for (int j = 0; j < count; j++) {
            final double a = scales[start + j];
            double[] w;
            int window = 0;
            if (sum) {
                // g(d) = psi(d / a) / sqrt(a), d = -m/2 + 1 .. m/2, cut at the outermost non-zero entries;
                // w[k] = g(dMax - k), the window starts at tau - dMax
                final int dLo = m > 1 ? -(m / 2) + 1 : 0, dHi = m / 2;
                double[] g = new double[dHi - dLo + 1];
                for (int d = dLo; d <= dHi; d++) {
                    g[d - dLo] = wavelet.psi(d / a) / Math.sqrt(a);   // i / scale, (i - fftSize) / scale: :570-575
                }
                int lo = 0, hi = g.length - 1;
                while (hi > lo && g[hi] == 0.0) hi--;
                while (lo < hi && g[lo] == 0.0) lo++;
                w = new double[hi - lo + 1];
                for (int k = 0; k < w.length; k++) w[k] = g[hi - k];
                window = -(dLo + hi);
                wts[2 * j] = weights[j] / a;   // :238
            } else {
                // reconstructionKernel (:359-374): (1.0 / sqrt(a)) * psi((t - b) / a), index t - b + n - 1
                final double scaleFactor = 1.0 / Math.sqrt(a);
                w = new double[2 * n - 1];
                for (int d = -(n - 1); d <= n - 1; d++) w[d + n - 1] = scaleFactor * wavelet.psi(d / a);
                wts[2 * j] = weights[j];
            }
            wts[2 * j + 1] = a;
            tables[j] = w;
            desc[4 * j] = total;
            desc[4 * j + 1] = w.length;
            desc[4 * j + 2] = window;
            desc[4 * j + 3] = start + j;
            total = Math.addExact(total, w.length);
        }
        double[] taps = new double[total];
        for (int j = 0; j < count; j++) System.arraycopy(tables[j], 0, taps, (int) desc[4 * j], tables[j].length);

        double[][] planeRows = new double[Math.multiplyExact(batch, numPlanes)][];
        for (int b = 0; b < batch; b++) {
            if (results[b] == null) throw new IllegalArgumentException("CWT result cannot be null");
            final double[][] coeffs = results[b].getCoefficients();
            if (coeffs == null || coeffs.length != numPlanes) {
                throw new IllegalArgumentException("every CWT result of a batch must hold the same scales");
            }
            System.arraycopy(coeffs, 0, planeRows, b * numPlanes, numPlanes);
        }
        double[] out = new double[Math.multiplyExact(batch, n)];
        AmdNative.check(AmdNative.icwtAoS(AmdRuntime.ctx(), planeRows, numPlanes, desc, wts, taps,
                sum ? AmdNative.ICWT_SUM : AmdNative.ICWT_DIRECT, sum ? m : 0, admissibilityConstant,
                sum ? AmdRuntime.FMA : 0, out));
        double[][] rows = new double[batch][n];
        for (int b = 0; b < batch; b++) System.arraycopy(out, b * n, rows[b], 0, n);
        return rows;
    }

    /** calculateLogScaleWeights (:411-453). */
    private static double[] logScaleWeights(double[] scales, int start, int end) {
        final int n = end - start;
        for (int i = start; i < end; i++) {
            if (scales[i] <= 0) {
                throw new IllegalArgumentException("Scale values must be positive for logarithmic integration. "
                        + "Found non-positive scale at index " + i + ": " + scales[i]);
            }
        }
        double[] weights = new double[n];
        if (n == 1) {
            weights[0] = scales[start];
            return weights;
        }
        for (int i = 0; i < n; i++) {
            if (i == 0) {
                weights[i] = Math.log(scales[start + 1] / scales[start]) / 2.0;
            } else if (i == n - 1) {
                weights[i] = Math.log(scales[start + i] / scales[start + i - 1]) / 2.0;
            } else {
                weights[i] = Math.log(scales[start + i + 1] / scales[start + i - 1]) / 2.0;
            }
        }
        return weights;
    }

    /** The smallest power of two >= n, 1 for n <= 1 (:591-600). */
    private static int nextPowerOfTwo(int n) {
        return n <= 1 ? 1 : Integer.highestOneBit(n - 1) << 1;
    }
}
