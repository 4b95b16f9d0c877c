package com.morphiqlabs.wavelet.amd;

import com.morphiqlabs.wavelet.api.ComplexContinuousWavelet;
import com.morphiqlabs.wavelet.api.ContinuousWavelet;
import com.morphiqlabs.wavelet.cwt.CWTConfig;
import com.morphiqlabs.wavelet.cwt.CWTResult;
import com.morphiqlabs.wavelet.cwt.ComplexMatrix;
import com.morphiqlabs.wavelet.cwt.ScaleSpace;

/**
 * MI355X drop-in for {@code CWTTransform.analyze} (cwt/CWTTransform.java:71-79), for one signal or a batch of
 * signals in one engine call, over the {@code cwtAoS} native (include/vectorwave_amd.h vw_cwt_f64).
 *
 * <p>The engine computes, per scale, the fixed-order correlation of every row with a table; this class builds the
 * tables with the wavelet's own {@code psi} / {@code psiImaginary}, evaluated exactly as the reference's loops
 * evaluate them, and picks the branch as {@code analyze} does:
 * <ul>
 * <li>direct (analyzeDirect :120-169 / analyzeDirectComplex :174-218; complex wavelets always, real ones when not
 * {@code config.shouldUseFFT(n)}): {@code w[k] = psi(-(k - H)/s) / sqrtScale}, window start {@code -H}, the padding
 * strategy as the extension.  Without FMA the coefficients are the reference's bit for bit.</li>
 * <li>FFT (analyzeFFT :223-318; real wavelets when {@code shouldUseFFT(n)}): the sum that branch's FFTs evaluate,
 * {@code (sum_k psi((k - H)/s) z[(i + H + k) mod M]) / sqrtScale} over the signal zero-padded to the FFT size M --
 * the window starts at {@code i + H} as the reference's extraction does (:304-311).  The engine evaluates the sum
 * directly, so the result differs from the reference's by its FFT's rounding (about 1e-15 relative); non-finite
 * samples, which the reference's FFT spreads over every output, are unspecified here.</li>
 * </ul>
 * {@code H = max(16, ceil(8 s bandwidth)) / 2} (:774-794).  Validation as validateInputs (:450-469).
 *
 * <p>Not here: analyzeComplex, the inverse transforms, the adaptive scale selectors, the cwt/finance analyzers.
 *
 * <p>Not built or run in this repository (no JDK in its build image): INTEGRATION.md section 2.
 */
public final class AmdCWTTransform {
    private static final int WAVELET_SUPPORT_FACTOR = 8;  // CWTTransform.java:29

    private final ContinuousWavelet wavelet;
    private final CWTConfig config;

    public AmdCWTTransform(ContinuousWavelet wavelet) {
        this(wavelet, CWTConfig.defaultConfig());
    }

    public AmdCWTTransform(ContinuousWavelet wavelet, CWTConfig config) {
        if (wavelet == null) throw new IllegalArgumentException("Wavelet cannot be null");
        if (config == null) throw new IllegalArgumentException("Config cannot be null");
        this.wavelet = wavelet;
        this.config = config;
    }

    /** {@code CWTTransform.analyze(signal, scales)}. */
    public CWTResult analyze(double[] signal, double[] scales) {
        if (signal == null) throw new IllegalArgumentException("Signal cannot be null");
        return analyze(new double[][] {signal}, scales)[0];
    }

    public CWTResult analyze(double[] signal, ScaleSpace scaleSpace) {
        if (scaleSpace == null) throw new IllegalArgumentException("ScaleSpace cannot be null");
        return analyze(signal, scaleSpace.getScales());
    }

    /** {@code analyze(signals[b], scales)} for every signal (all of one length), one engine call for the batch. */
    public CWTResult[] analyze(double[][] signals, double[] scales) {
        if (signals == null) throw new IllegalArgumentException("Signal cannot be null");
        if (signals.length == 0 || signals[0] == null || signals[0].length == 0) {
            throw new IllegalArgumentException("Signal cannot be empty");
        }
        if (scales == null) throw new IllegalArgumentException("Scales cannot be null");
        if (scales.length == 0) throw new IllegalArgumentException("Scales cannot be empty");
        for (double scale : scales) {
            if (scale <= 0) throw new IllegalArgumentException("All scales must be positive");
        }
        final int batch = signals.length, n = signals[0].length, numScales = scales.length;
        final boolean complex = wavelet.isComplex();
        final boolean fft = config.shouldUseFFT(n) && !complex;
        final ComplexContinuousWavelet cw = wavelet instanceof ComplexContinuousWavelet c ? c : null;

        // the tables: w_s[k], k = 0 .. 2 H_s
        long[] desc = new long[3 * numScales];
        double[] divisors = new double[numScales];
        int total = 0, maxSupport = 0;
        for (int s = 0; s < numScales; s++) {
            final int support = waveletSupport(scales[s]), half = support / 2;
            maxSupport = Math.max(maxSupport, support);
            desc[3 * s] = total;
            desc[3 * s + 1] = 2L * half + 1;
            desc[3 * s + 2] = fft ? half : -half;
            total = Math.addExact(total, 2 * half + 1);
        }
        double[] tapsRe = new double[total];
        double[] tapsIm = complex ? new double[total] : null;
        for (int s = 0; s < numScales; s++) {
            final double scale = scales[s];
            final double sqrtScale = config.isNormalizeAcrossScales() ? Math.sqrt(scale) : 1.0;
            final int half = (int) (desc[3 * s + 1] / 2), at = (int) desc[3 * s];
            divisors[s] = fft ? sqrtScale : 1.0;
            for (int k = 0; k <= 2 * half; k++) {
                if (fft) {
                    tapsRe[at + k] = wavelet.psi((k - half) / scale);                 // :331-336
                } else {
                    final int t = k - half;
                    tapsRe[at + k] = wavelet.psi(-t / scale) / sqrtScale;             // :153, :203
                    if (cw != null) tapsIm[at + k] = cw.psiImaginary(-t / scale) / sqrtScale;  // :208
                }
            }
        }
        long wrap = 0;
        int ext = switch (config.getPaddingStrategy()) {
            case ZERO -> AmdNative.CWT_ZERO;
            case REFLECT -> AmdNative.CWT_REFLECT;
            case SYMMETRIC -> AmdNative.CWT_SYMMETRIC;
            case PERIODIC -> AmdNative.CWT_PERIODIC;
        };
        if (fft) {  // :227-238
            ext = AmdNative.CWT_WRAP_ZERO;
            wrap = nextPowerOfTwo(n + maxSupport - 1);
            if (config.getFFTSize() > 0) wrap = Math.max(config.getFFTSize(), wrap);
        }

        final int plane = Math.multiplyExact(Math.multiplyExact(batch, numScales), n);
        double[] outRe = new double[plane];
        double[] outIm = complex ? new double[plane] : null;
        AmdNative.check(AmdNative.cwtAoS(AmdRuntime.ctx(), signals, desc, divisors, tapsRe, tapsIm, ext, wrap,
                AmdRuntime.FMA, outRe, outIm));

        CWTResult[] results = new CWTResult[batch];
        for (int b = 0; b < batch; b++) {
            double[][] re = new double[numScales][n];
            double[][] im = complex ? new double[numScales][n] : null;
            for (int s = 0; s < numScales; s++) {
                System.arraycopy(outRe, (b * numScales + s) * n, re[s], 0, n);
                if (complex) System.arraycopy(outIm, (b * numScales + s) * n, im[s], 0, n);
            }
            results[b] = complex ? new CWTResult(new ComplexMatrix(re, im), scales, wavelet)
                                 : new CWTResult(re, scales, wavelet);
        }
        return results;
    }

    /** CWTTransform.getWaveletSupport (:774-783). */
    private int waveletSupport(double scale) {
        return Math.max(16, (int) Math.ceil(WAVELET_SUPPORT_FACTOR * scale * wavelet.bandwidth()));
    }

    /** The smallest power of two >= n, 1 for n <= 1: the values of CWTTransform.nextPowerOfTwo (:757-766). */
    private static int nextPowerOfTwo(int n) {
        return n <= 1 ? 1 : Integer.highestOneBit(n - 1) << 1;
    }
}
