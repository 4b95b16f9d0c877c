package com.morphiqlabs.wavelet.amd;

import com.morphiqlabs.financial.FinancialAnalysisConfig;
import com.morphiqlabs.financial.FinancialAnalyzer.VolatilityClassification;
import com.morphiqlabs.financial.FinancialConfig;
import com.morphiqlabs.wavelet.api.BoundaryMode;
import com.morphiqlabs.wavelet.api.Daubechies;
import com.morphiqlabs.wavelet.api.Haar;
import com.morphiqlabs.wavelet.api.Wavelet;

/**
 * MI355X drop-in for com.morphiqlabs.financial.FinancialAnalyzer (FinancialAnalyzer.java:52-234) and
 * FinancialWaveletAnalyzer (FinancialWaveletAnalyzer.java:82-212), over the {@code finAnalyzeAoS},
 * {@code finSharpeAoS} and {@code finWaveletSharpeAoS} natives (include/vectorwave_amd.h vw_fin_*).
 *
 * <p>The single-series methods keep the reference's signatures and results bit for bit: returns as
 * calculateReturns computes them, the level-1 MODWT (DB4, PERIODIC for the analysis; Haar, PERIODIC by
 * default for the Sharpe ratios), then the reference's sequential sums.  The batch methods do the same for every
 * row of a {@code double[][]} in one engine launch: a row is read once and about 40 bytes come back, instead of
 * both coefficient planes.  {@code treeSums} replaces the sequential sums by tree reductions (faster, equal
 * within rounding, not bit for bit).  Fused multiply-add is never used here: it would turn the exactly-zero
 * details of quantised prices into signed values and change the asymmetry counts.
 *
 * <p>Exceptions: IllegalArgumentException with the reference's messages for short series and non-finite
 * prices, InvalidSignalException where the reference's transform.forward rejects a non-finite return.
 *
 * <p>Not built or run in this repository (no JDK in its build image): INTEGRATION.md section 2.
 */
public final class AmdFinancialAnalyzer {
    /** One launch's results, one entry per price row. */
    public record Analysis(double[] crashAsymmetry, double[] volatility, double[] regimeTrend, boolean[] anomalies,
                           double[] detailStdDev) {}

    private final FinancialAnalysisConfig config;
    private final FinancialConfig financialConfig;
    private final Wavelet analysisWavelet = Daubechies.DB4;  // FinancialAnalyzer.java:37
    private final Wavelet sharpeWavelet;
    private final int sharpeBoundary;

    /** FinancialAnalyzer(config) (:32-38); the Sharpe methods need the other constructor. */
    public AmdFinancialAnalyzer(FinancialAnalysisConfig config) {
        this(config, null, Haar.INSTANCE, BoundaryMode.PERIODIC);
    }

    /** FinancialWaveletAnalyzer(config) (:48-54): Haar, PERIODIC. */
    public AmdFinancialAnalyzer(FinancialAnalysisConfig config, FinancialConfig financialConfig) {
        this(config, financialConfig, Haar.INSTANCE, BoundaryMode.PERIODIC);
    }

    /** FinancialWaveletAnalyzer(config, transform) (:63-72), the transform given by its wavelet and boundary mode. */
    public AmdFinancialAnalyzer(FinancialAnalysisConfig config, FinancialConfig financialConfig, Wavelet wavelet,
                                BoundaryMode boundaryMode) {
        if (config == null) {
            throw new IllegalArgumentException("Configuration cannot be null");
        }
        if (wavelet == null || boundaryMode == null) {
            throw new IllegalArgumentException("Wavelet transform cannot be null");
        }
        this.config = config;
        this.financialConfig = financialConfig;
        this.sharpeWavelet = wavelet;
        this.sharpeBoundary = AmdNative.boundary(boundaryMode);
    }

    public FinancialAnalysisConfig getConfig() {
        return config;
    }

    // ---- FinancialAnalyzer ------------------------------------------------------------------------

    /** analyzeCrashAsymmetry(prices) (:52-91). */
    public double analyzeCrashAsymmetry(double[] prices) {
        return analyzeOne(prices).crashAsymmetry()[0];
    }

    /** analyzeVolatility(prices) (:103-120). */
    public double analyzeVolatility(double[] prices) {
        return analyzeOne(prices).volatility()[0];
    }

    /** analyzeRegimeTrend(prices) (:132-154). */
    public double analyzeRegimeTrend(double[] prices) {
        return analyzeOne(prices).regimeTrend()[0];
    }

    /** detectAnomalies(prices) (:166-198). */
    public boolean detectAnomalies(double[] prices) {
        return analyzeOne(prices).anomalies()[0];
    }

    /** All four metrics (and the detail standard deviation) of every row, one launch; the reference's sums. */
    public Analysis analyzeBatch(double[][] prices) {
        return analyzeBatch(prices, false);
    }

    /** As {@link #analyzeBatch(double[][])}; {@code treeSums}: tree reductions instead of sequential sums. */
    public Analysis analyzeBatch(double[][] prices, boolean treeSums) {
        if (prices == null) {
            throw new IllegalArgumentException("Prices cannot be null");
        }
        final int batch = prices.length;
        double[] out = new double[5 * batch];
        AmdNative.check(AmdNative.finAnalyzeAoS(AmdRuntime.ctx(), prices, analysisWavelet.lowPassDecomposition(),
                analysisWavelet.highPassDecomposition(), config.getAnomalyDetectionThreshold(),
                AmdNative.FLAG_VALIDATE | (treeSums ? AmdNative.FLAG_TREE_SUMS : 0), out));
        double[][] plane = new double[5][batch];
        for (int k = 0; k < 5; k++) {
            System.arraycopy(out, k * batch, plane[k], 0, batch);
        }
        boolean[] flags = new boolean[batch];
        for (int b = 0; b < batch; b++) {
            flags[b] = plane[3][b] != 0.0;
        }
        return new Analysis(plane[0], plane[1], plane[2], flags, plane[4]);
    }

    private Analysis analyzeOne(double[] prices) {
        if (prices == null) {
            throw new IllegalArgumentException("Prices cannot be null");  // validatePrices :271-273
        }
        return analyzeBatch(new double[][] {prices}, false);
    }

    /** classifyVolatility(volatility) (:206-214). */
    public VolatilityClassification classifyVolatility(double volatility) {
        if (volatility < config.getVolatilityLowThreshold()) {
            return VolatilityClassification.LOW;
        } else if (volatility > config.getVolatilityHighThreshold()) {
            return VolatilityClassification.HIGH;
        }
        return VolatilityClassification.NORMAL;
    }

    /** isCrashRisk(asymmetry) (:222-224). */
    public boolean isCrashRisk(double asymmetry) {
        return asymmetry > config.getCrashAsymmetryThreshold();
    }

    /** isRegimeShift(trendChange) (:232-234). */
    public boolean isRegimeShift(double trendChange) {
        return trendChange > config.getRegimeTrendThreshold();
    }

    // ---- FinancialWaveletAnalyzer -------------------------------------------------------------------

    /** calculateSharpeRatio(returns) (:82-84). */
    public double calculateSharpeRatio(double[] returns) {
        return calculateSharpeRatio(returns, riskFreeRate());
    }

    /** calculateSharpeRatio(returns, riskFreeRate) (:95-124). */
    public double calculateSharpeRatio(double[] returns, double riskFreeRate) {
        return sharpeBatch(one(returns), riskFreeRate, false, false)[0];
    }

    /** calculateWaveletSharpeRatio(returns) (:151-153). */
    public double calculateWaveletSharpeRatio(double[] returns) {
        return calculateWaveletSharpeRatio(returns, riskFreeRate());
    }

    /** calculateWaveletSharpeRatio(returns, riskFreeRate) (:166-212). */
    public double calculateWaveletSharpeRatio(double[] returns, double riskFreeRate) {
        return sharpeBatch(one(returns), riskFreeRate, true, false)[0];
    }

    /** calculateSharpeRatio of every row, one launch. */
    public double[] calculateSharpeRatioBatch(double[][] returns, double riskFreeRate, boolean treeSums) {
        return sharpeBatch(returns, riskFreeRate, false, treeSums);
    }

    /** calculateWaveletSharpeRatio of every row, one launch (PERIODIC; the other modes run three). */
    public double[] calculateWaveletSharpeRatioBatch(double[][] returns, double riskFreeRate, boolean treeSums) {
        return sharpeBatch(returns, riskFreeRate, true, treeSums);
    }

    private double riskFreeRate() {
        if (financialConfig == null) {
            throw new IllegalArgumentException("Financial configuration cannot be null");
        }
        return financialConfig.getRiskFreeRate();
    }

    private static double[][] one(double[] returns) {
        if (returns == null) {
            throw new IllegalArgumentException("Returns array cannot be null");  // :96-98, :167-169
        }
        if (returns.length == 0) {
            throw new IllegalArgumentException("Returns array cannot be empty");  // :99-101, :170-172
        }
        return new double[][] {returns};
    }

    private double[] sharpeBatch(double[][] returns, double riskFreeRate, boolean wavelet, boolean treeSums) {
        if (returns == null) {
            throw new IllegalArgumentException("Returns array cannot be null");
        }
        double[] out = new double[returns.length];
        final int flags = treeSums ? AmdNative.FLAG_TREE_SUMS : 0;
        if (wavelet) {
            // transform.forward validates its input (MODWTTransform.java:369-414)
            AmdNative.check(AmdNative.finWaveletSharpeAoS(AmdRuntime.ctx(), returns,
                    sharpeWavelet.lowPassDecomposition(), sharpeWavelet.highPassDecomposition(), sharpeBoundary,
                    riskFreeRate, flags | AmdNative.FLAG_VALIDATE, out));
        } else {
            AmdNative.check(AmdNative.finSharpeAoS(AmdRuntime.ctx(), returns, riskFreeRate, flags, out));
        }
        return out;
    }
}
