package com.morphiqlabs.wavelet.amd;

import com.morphiqlabs.wavelet.api.BoundaryMode;
import com.morphiqlabs.wavelet.api.Wavelet;
import com.morphiqlabs.wavelet.exception.ErrorCode;
import com.morphiqlabs.wavelet.exception.InvalidArgumentException;
import com.morphiqlabs.wavelet.exception.InvalidSignalException;
import com.morphiqlabs.wavelet.modwt.MultiLevelMODWTResult;

/**
 * MI355X drop-in for core/modwt/MultiLevelMODWTTransform.java: {@code decompose}, {@code reconstruct},
 * {@code reconstructFromLevel}, {@code reconstructLevels} with the reference's semantics -- level cap
 * ({@code getMaximumLevels}, :455-501), non-finite input rejected with VAL_NON_FINITE_VALUES, PERIODIC /
 * ZERO_PADDING / SYMMETRIC boundaries (K4 / K5 / K6, :554-645, SymmetricAlignmentStrategy), the FFT
 * switch region reproduced (:710-757) -- plus batch forms over {@code double[][]} that the reference runs
 * one signal at a time.  EXACT accumulation by default: the reference's results bit for bit
 * ({@link AmdRuntime}).
 *
 * <p>Not built or run in this repository (no JDK in its build image): INTEGRATION.md section 2.
 */
public final class AmdMultiLevelMODWT {
    private final Wavelet wavelet;
    private final BoundaryMode boundaryMode;
    private final int boundary;

    /** MultiLevelMODWTTransform(Wavelet, BoundaryMode) (:181-193). */
    public AmdMultiLevelMODWT(Wavelet wavelet, BoundaryMode boundaryMode) {
        if (wavelet == null) throw new NullPointerException("wavelet cannot be null");
        if (boundaryMode == null) throw new NullPointerException("boundaryMode cannot be null");
        this.wavelet = wavelet;
        this.boundaryMode = boundaryMode;
        this.boundary = AmdNative.boundary(boundaryMode);  // CONSTANT -> CFG_UNSUPPORTED_BOUNDARY_MODE
    }

    public Wavelet getWavelet() {
        return wavelet;
    }

    public BoundaryMode getBoundaryMode() {
        return boundaryMode;
    }

    /** getMaximumLevels (:455-501): largest J <= 9 whose upsampled filter fits the signal. */
    public int getMaximumLevels(int signalLength) {
        return AmdNative.maxLevels(signalLength, wavelet.lowPassDecomposition().length);
    }

    /** decompose(signal) (:195-207): as many levels as the signal allows. */
    public MultiLevelMODWTResult decompose(double[] signal) {
        if (signal == null) throw new NullPointerException("signal cannot be null");
        return decompose(signal, getMaximumLevels(signal.length));
    }

    /** decompose(signal, levels) (:209-255). */
    public MultiLevelMODWTResult decompose(double[] signal, int levels) {
        return decomposeBatch(new double[][] {signal}, levels)[0];
    }

    /**
     * One call for a batch of equal-length signals: element b equals {@code decompose(signals[b], levels)}.
     * Validation as decompose, per signal; the error names the first offending signal of the batch (the
     * native side may already have transformed earlier row chunks -- their results are discarded with the
     * exception).  reconstruct* validate nothing, as the reference's (FLAG_REF_NONFINITE: NaN / +-Inf in a
     * result spread as the reference's loops spread them).
     */
    public MultiLevelMODWTResult[] decomposeBatch(double[][] signals, int levels) {
        final int n = equalRows(signals);
        final int batch = signals.length;
        if (levels < 1 || levels > getMaximumLevels(n)) {
            // the reference's order (:209-240): non-finite values, empty signal, then the level range
            for (int b = 0; b < batch; b++) {
                for (int t = 0; t < n; t++) {
                    if (!Double.isFinite(signals[b][t])) {
                        throw new InvalidSignalException(ErrorCode.VAL_NON_FINITE_VALUES,
                                "signal contains non-finite values [signal " + b + ", index " + t + "]");
                    }
                }
            }
            if (n == 0) {
                throw new InvalidSignalException(ErrorCode.VAL_EMPTY, "Signal cannot be empty for multi-level MODWT");
            }
            throw new InvalidArgumentException(ErrorCode.CFG_INVALID_DECOMPOSITION_LEVEL,
                    "Invalid number of decomposition levels: " + levels + " (valid: 1.." + getMaximumLevels(n) + ")");
        }
        double[][][] det = new double[levels][batch][n];
        double[][] app = new double[batch][n];
        final int flags = AmdNative.FLAG_CORE_LEVELS | AmdNative.FLAG_VALIDATE | AmdNative.FLAG_FFT_SWITCH
                | AmdRuntime.FMA;
        // (a BiorthogonalWavelet, whose two filters differ in length, goes through modwtForwardBiAoS)
        AmdNative.check(AmdNative.forwardAoS(AmdRuntime.ctx(), signals, wavelet.lowPassDecomposition(),
                wavelet.highPassDecomposition(), AmdNative.waveletId(wavelet), boundary, levels, flags, det, app));
        MultiLevelMODWTResult[] out = new MultiLevelMODWTResult[batch];
        for (int b = 0; b < batch; b++) {
            double[][] d = new double[levels][];
            for (int l = 0; l < levels; l++) d[l] = det[l][b];
            out[b] = new AmdMultiLevelResult(d, app[b]);
        }
        return out;
    }

    /**
     * Energy per level of {@code decompose(signals[b], levels)} for every signal, without the coefficients:
     * {@code [B][levels + 1]} in getRelativeEnergyDistribution's order {@code [approx, d1..dJ]}
     * (MultiLevelMODWTResultImpl :91-117, computeEnergy :211-216; sequential sums, the reference's bits).
     * Validation as decomposeBatch, by the engine.
     */
    public double[][] energyBatch(double[][] signals, int levels) {
        final int n = equalRows(signals);
        final int batch = signals.length;
        double[] flat = new double[Math.multiplyExact(levels + 1, batch)];
        final int flags = AmdNative.FLAG_CORE_LEVELS | AmdNative.FLAG_VALIDATE | AmdNative.FLAG_FFT_SWITCH
                | AmdRuntime.FMA;
        AmdNative.check(AmdNative.modwtEnergyAoS(AmdRuntime.ctx(), signals, wavelet.lowPassDecomposition(),
                wavelet.highPassDecomposition(), AmdNative.waveletId(wavelet), boundary, levels, flags, flat));
        return perSignal(flat, levels + 1, batch);
    }

    /** getRelativeEnergyDistribution (:121-138) of every signal: {@code [B][levels + 1]}. */
    public double[][] relativeEnergyBatch(double[][] signals, int levels) {
        return relative(energyBatch(signals, levels));
    }

    /** flat [planes][batch] -> [batch][planes] */
    static double[][] perSignal(double[] flat, int planes, int batch) {
        double[][] out = new double[batch][planes];
        for (int k = 0; k < planes; k++) {
            for (int b = 0; b < batch; b++) out[b][k] = flat[k * batch + b];
        }
        return out;
    }

    /** total = approx; total += d_1 .. d_J; each energy / total; all zeros when total == 0.0 (:121-138). */
    static double[][] relative(double[][] energies) {
        double[][] out = new double[energies.length][];
        for (int b = 0; b < energies.length; b++) {
            final double[] e = energies[b];
            double total = e[0];
            for (int j = 1; j < e.length; j++) total += e[j];
            out[b] = new double[e.length];
            if (total == 0.0) continue;
            for (int j = 0; j < e.length; j++) out[b][j] = e[j] / total;
        }
        return out;
    }

    /** reconstruct (:339-349): the cascade J..1. */
    public double[] reconstruct(MultiLevelMODWTResult result) {
        if (result == null) throw new NullPointerException("result cannot be null");
        return inverse(result, ~0, false);
    }

    /** reconstructFromLevel (:361-386): details finer than startLevel are zero. */
    public double[] reconstructFromLevel(MultiLevelMODWTResult result, int startLevel) {
        if (result == null) throw new NullPointerException("result cannot be null");
        final int J = result.getLevels();
        if (startLevel < 1 || startLevel > J) {
            throw new InvalidArgumentException("Invalid start level: " + startLevel + ". Must be between 1 and " + J);
        }
        int mask = 0;
        for (int lev = startLevel; lev <= J; lev++) mask |= 1 << (lev - 1);
        return inverse(result, mask, false);
    }

    /** reconstructLevels (:398-446): only details in [minLevel, maxLevel]; the approximation only if J <= maxLevel. */
    public double[] reconstructLevels(MultiLevelMODWTResult result, int minLevel, int maxLevel) {
        if (result == null) throw new NullPointerException("result cannot be null");
        final int J = result.getLevels();
        if (minLevel < 1 || maxLevel > J || minLevel > maxLevel) {
            throw new InvalidArgumentException(ErrorCode.CFG_INVALID_DECOMPOSITION_LEVEL,
                    "Invalid level range for partial reconstruction");
        }
        int mask = 0;
        for (int lev = minLevel; lev <= maxLevel; lev++) mask |= 1 << (lev - 1);
        return inverse(result, mask, J > maxLevel);
    }

    /**
     * Multiresolution analysis of a decomposition: {@code [J + 1][N]}, row 0 the smooth
     * ({@code reconstructLevels}' result with every detail zeroed and the approximation kept), row j detail
     * component j (only d_j kept, the approximation zeroed) -- what J + 1 calls of the masked inverse give, bit for
     * bit, from one engine call; the rows add up to {@code reconstruct(result)}.  Like reconstruct* it validates
     * nothing and carries FLAG_REF_NONFINITE (the engine then loops over the masked inverses);
     * {@code finite = true} promises finite coefficients and lets the one-launch kernel run.  A
     * BiorthogonalWavelet loops over the two-length inverse.
     */
    public double[][] mra(MultiLevelMODWTResult result, boolean finite) {
        if (result == null) throw new NullPointerException("result cannot be null");
        final int J = result.getLevels();
        final int n = result.getSignalLength();
        final double[] rlo = wavelet.lowPassReconstruction(), rhi = wavelet.highPassReconstruction();
        double[][] out = new double[J + 1][];
        if (rlo.length != rhi.length) {
            for (int c = 0; c <= J; c++) out[c] = inverse(result, c == 0 ? 0 : 1 << (c - 1), c != 0);
            return out;
        }
        double[][][] d = new double[J][1][];
        for (int l = 1; l <= J; l++) d[l - 1][0] = result.getDetailCoeffsAtLevel(l);
        double[][] a = {result.getApproximationCoeffs()};
        double[] flat = new double[Math.multiplyExact(J + 1, n)];
        final int flags = AmdNative.FLAG_CORE_LEVELS | (finite ? 0 : AmdNative.FLAG_REF_NONFINITE) | AmdRuntime.FMA;
        AmdNative.check(AmdNative.mraPlanesAoS(AmdRuntime.ctx(), d, a, rlo, rhi, AmdNative.waveletId(wavelet), boundary,
                flags, flat));
        for (int c = 0; c <= J; c++) {
            out[c] = new double[n];
            System.arraycopy(flat, c * n, out[c], 0, n);
        }
        return out;
    }

    /**
     * {@code mra(decompose(signals[b], levels), finite)} for every signal, one engine call for the batch:
     * {@code [B][levels + 1][N]}.  Validation as decomposeBatch, by the engine (FLAG_VALIDATE keeps the call on
     * the masked inverses; {@code finite = true} trusts the caller instead).  Equal-length banks only.
     */
    public double[][][] mraBatch(double[][] signals, int levels, boolean finite) {
        final int n = equalRows(signals);
        final int batch = signals.length;
        double[] flat = new double[Math.multiplyExact(Math.multiplyExact(levels + 1, batch), n)];
        final int flags = AmdNative.FLAG_CORE_LEVELS | AmdNative.FLAG_FFT_SWITCH | AmdRuntime.FMA
                | (finite ? 0 : AmdNative.FLAG_VALIDATE | AmdNative.FLAG_REF_NONFINITE);
        AmdNative.check(AmdNative.mraAoS(AmdRuntime.ctx(), signals, wavelet.lowPassDecomposition(),
                wavelet.highPassDecomposition(), AmdNative.waveletId(wavelet), boundary, levels, flags, flat));
        double[][][] out = new double[batch][levels + 1][n];
        for (int c = 0; c <= levels; c++) {
            for (int b = 0; b < batch; b++) System.arraycopy(flat, (c * batch + b) * n, out[b][c], 0, n);
        }
        return out;
    }

    /** {@code mra(result, false)}: the reference's NaN / +-Inf spread kept. */
    public double[][] mra(MultiLevelMODWTResult result) {
        return mra(result, false);
    }

    private double[] inverse(MultiLevelMODWTResult r, int mask, boolean approxZero) {
        final int J = r.getLevels();
        final int n = r.getSignalLength();
        final double[] rlo = wavelet.lowPassReconstruction(), rhi = wavelet.highPassReconstruction();
        if (rlo.length != rhi.length) {
            // a BiorthogonalWavelet: the two-length native takes whole planes, so a masked level is passed as the
            // zero row the engine would read for it, and a dropped approximation as a zero row
            double[][][] d = new double[J][1][];
            for (int l = 1; l <= J; l++) {
                d[l - 1][0] = ((mask >>> (l - 1)) & 1) != 0 ? r.getDetailCoeffsAtLevel(l) : new double[n];
            }
            double[][] a = {approxZero ? new double[n] : r.getApproximationCoeffs()};
            double[][] out = new double[1][n];
            AmdNative.check(AmdNative.modwtInverseBiAoS(AmdRuntime.ctx(), d, a, rlo, rhi, AmdNative.waveletId(wavelet),
                    boundary, AmdNative.FLAG_CORE_LEVELS | AmdNative.FLAG_REF_NONFINITE | AmdRuntime.FMA, out));
            return out[0];
        }
        double[] det = new double[Math.multiplyExact(J, n)];
        for (int l = 1; l <= J; l++) {
            System.arraycopy(r.getDetailCoeffsAtLevel(l), 0, det, (l - 1) * n, n);
        }
        double[] y = new double[n];
        AmdNative.check(AmdNative.modwtInverse(AmdRuntime.ctx(), det, r.getApproximationCoeffs(), 1, n,
                wavelet.lowPassReconstruction(), wavelet.highPassReconstruction(), AmdNative.waveletId(wavelet),
                boundary, J, mask, approxZero,
                AmdNative.FLAG_CORE_LEVELS | AmdNative.FLAG_REF_NONFINITE | AmdRuntime.FMA, y));
        return y;
    }

    static int equalRows(double[][] signals) {
        if (signals == null) throw new NullPointerException("signals cannot be null");
        if (signals.length == 0 || signals[0] == null) {
            throw new IllegalArgumentException("signals must be non-null and non-empty");
        }
        final int n = signals[0].length;
        for (int i = 1; i < signals.length; i++) {
            if (signals[i] == null || signals[i].length != n) {
                throw new IllegalArgumentException("all signals must be non-null and same length");
            }
        }
        return n;
    }
}
