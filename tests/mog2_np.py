"""numpy restatement of cv2.createBackgroundSubtractorMOG2(...).apply on 8-bit 3-channel images.

TEST INFRASTRUCTURE ONLY: never imported by the package.  PARITY UNPINNED: cv2 is absent here and the reference keeps no model
state, so this restates the published CPU path of OpenCV's bgfg_gaussmix2.cpp (BackgroundSubtractorMOG2Impl::apply,
MOG2Invoker, detectShadowGMM; Zivkovic's adaptive mixture).  Reference lines it stands for: background_subtraction.py:90-127
(train_MOG2_background_model) and :158 (`bg_model.apply(image, None, 0)`).

Constructor: history = h > 0 ? h : 500; varThreshold = double((float)(v > 0 ? v : 16)); nmixtures 5, backgroundRatio 0.9f,
varThresholdGen 9f, varInit 15f, varMin 4f, varMax 75f, complexityReductionThreshold (fCT) 0.05f, shadowValue 127,
shadowThreshold (tau) 0.5f -- all of them keyword arguments here.
apply(image, learningRate): the model (per pixel a u8 nmodes and K x {weight, variance, mean[3]} float32, all zero) starts over
on the first frame, on learningRate >= 1 and on a change of image size; ++nframes; lr = learningRate if learningRate >= 0 and
nframes > 1 else 1 / min(2 nframes, history) (double); alphaT = (float)lr, alpha1 = 1 - alphaT, prune = (float)(-lr * fCT).
Per pixel, float32, left to right, no contraction (MAX / MIN are OpenCV's macros, NaN goes through them as in C):

  background = fits = false; n = nmodes; total = 0
  for m = 0; m < n; m++:                                      (n shrinks when a mode is pruned)
      weight = alpha1 * w[m] + prune; swaps = 0
      if !fits:
          d = mean[m] - data; dist2 = d0 d0 + d1 d1 + d2 d2
          if total < TB and dist2 < Tb var[m]: background = true
          if dist2 < Tg var[m]: fits = true; weight += alphaT; k = alphaT / weight; mean[m] -= k d
                                var[m] = MIN(MAX(var + k (dist2 - var), varMin), varMax)
                                bubble m up while !(weight < w[i-1]) (swaps counts the moves)
      if weight < -prune: weight = 0; n--
      w[m - swaps] = weight; total += weight
  inv = |total| > FLT_EPSILON ? 1 / total : 0; w[m] *= inv for m < n
  if !fits and alphaT > 0: m = n == K ? K-1 : n++; w[m] = 1 if n == 1 else alphaT (and w[i] *= alpha1 for i < n-1)
                           mean[m] = data; var[m] = varInit; bubble m up while !(alphaT < w[i-1])
  nmodes = n; mask = background ? 0 : detectShadows and shadow(data, n) ? shadowValue : 255
  shadow: for m < n: num = sum data mean[m]; den = sum mean[m]^2 (from 0.0f, channel order); den == 0 -> false
          if num <= den and num >= tau den: a = num / den; d2a = sum (a mean[m] - data)^2; d2a < Tb var a a -> true
          tw += w[m]; tw > TB -> false

State layout (the device's): float32 [5 K, H W], plane 5 k + f = field f (0 weight, 1 variance, 2..4 mean) of component k, and
u8 [H W] nmodes.  Components at k >= nmodes keep whatever was last written there.
"""
import numpy as np

F = np.float32
EPS = F(1.1920928955078125e-7)           # FLT_EPSILON
MAX_MIXTURES = 8


class MOG2:
    def __init__(self, history=500, varThreshold=16, detectShadows=True, nmixtures=5, backgroundRatio=0.9, varThresholdGen=9,
                 varInit=15, varMin=4, varMax=75, complexityReductionThreshold=0.05, shadowValue=127, shadowThreshold=0.5):
        assert 1 <= nmixtures <= MAX_MIXTURES
        self.history = int(history) if history > 0 else 500
        self.varThreshold = float(F(varThreshold if varThreshold > 0 else 16))
        self.detectShadows = bool(detectShadows)
        self.K = int(nmixtures)
        self.TB, self.Tg = F(backgroundRatio), F(varThresholdGen)
        self.varInit, self.varMin, self.varMax = F(varInit), F(varMin), F(varMax)
        self.fCT, self.tau = F(complexityReductionThreshold), F(shadowThreshold)
        self.shadowValue = int(shadowValue)
        self.nframes = 0
        self.shape = None
        self.state = None                # float32 [5 K, H W]
        self.nmodes = None               # uint8 [H W]
        self.stats = {}                  # how often the rarer branches ran (tests assert that they were exercised)

    def apply(self, image, learningRate=-1):
        img = np.asarray(image, dtype=np.uint8)
        assert img.ndim == 3 and img.shape[2] == 3
        if self.nframes == 0 or learningRate >= 1 or img.shape[:2] != self.shape:
            self.shape = img.shape[:2]
            self.state = np.zeros((5 * self.K, img.shape[0] * img.shape[1]), F)
            self.nmodes = np.zeros(img.shape[0] * img.shape[1], np.uint8)
            self.nframes = 0
        self.nframes += 1
        lr = learningRate if learningRate >= 0 and self.nframes > 1 else 1.0 / min(2 * self.nframes, self.history)
        alphaT = F(lr)
        prune = F(-lr * float(self.fCT))
        with np.errstate(all="ignore"):
            out = self._process(img.reshape(-1, 3).astype(F), alphaT, F(F(1) - alphaT), prune)
        return out.reshape(self.shape)

    def _bump(self, key, count):
        self.stats[key] = self.stats.get(key, 0) + int(count)

    def _process(self, pix, alphaT, alpha1, prune):
        K, TB, Tg, Tb = self.K, self.TB, self.Tg, F(self.varThreshold)
        st = self.state.reshape(K, 5, -1)
        w, var, mu = st[:, 0], st[:, 1], st[:, 2:5]           # views [K, n], [K, n], [K, 3, n]
        data = pix.T                                           # [3, n]
        npx = data.shape[1]
        n0 = np.minimum(self.nmodes.astype(np.int64), K)
        n = n0.copy()
        background = np.zeros(npx, bool)
        fits = np.zeros(npx, bool)
        total = np.zeros(npx, F)
        for m in range(K):
            act = m < n
            if not act.any():
                break
            weight = alpha1 * w[m] + prune
            swaps = np.zeros(npx, np.int64)
            probe = act & ~fits
            d = mu[m] - data
            dist2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            vm = var[m].copy()
            background |= probe & (total < TB) & (dist2 < Tb * vm)
            hit = probe & (dist2 < Tg * vm)
            if hit.any():
                fits |= hit
                weight = np.where(hit, weight + alphaT, weight)
                k = alphaT / weight
                for c in range(3):
                    mu[m, c] = np.where(hit, mu[m, c] - k * d[c], mu[m, c])
                vn = vm + k * (dist2 - vm)
                vn = np.where(vn < self.varMin, self.varMin, vn)
                vn = np.where(vn > self.varMax, self.varMax, vn)
                var[m] = np.where(hit, vn, var[m])
                moving = hit.copy()
                for i in range(m, 0, -1):
                    moving &= ~(weight < w[i - 1])
                    if not moving.any():
                        break
                    swaps += moving
                    for arr in (w, var, mu):
                        a, b = arr[i].copy(), arr[i - 1].copy()
                        arr[i] = np.where(moving, b, a)
                        arr[i - 1] = np.where(moving, a, b)
            pr = act & (weight < -prune)
            self._bump("pruned", pr.sum())
            weight = np.where(pr, F(0), weight)
            n = n - pr
            dst = m - swaps
            for j in range(m + 1):
                w[j] = np.where(act & (dst == j), weight, w[j])
            total = np.where(act, total + weight, total)
        inv = np.where(np.abs(total) > EPS, F(1) / total, F(0))
        for m in range(K):
            w[m] = np.where(m < n, w[m] * inv, w[m])
        new = ~fits & (alphaT > 0)
        full = new & (n == K)
        self._bump("replaced", full.sum())
        mnew = np.where(full, K - 1, n)
        n = np.where(new & ~full, n + 1, n)
        for j in range(K):
            at = new & (mnew == j)
            w[j] = np.where(at & (n == 1), F(1), np.where(at, alphaT, w[j]))
            var[j] = np.where(at, self.varInit, var[j])
            for c in range(3):
                mu[j, c] = np.where(at, data[c], mu[j, c])
            w[j] = np.where(new & (n != 1) & (j < n - 1), w[j] * alpha1, w[j])
        moving = new.copy()
        for i in range(K - 1, 0, -1):
            moving = np.where(i <= n - 1, moving & ~(alphaT < w[i - 1]), moving)
            sw = moving & (i <= n - 1)
            if sw.any():
                for arr in (w, var, mu):
                    a, b = arr[i].copy(), arr[i - 1].copy()
                    arr[i] = np.where(sw, b, a)
                    arr[i - 1] = np.where(sw, a, b)
        self.nmodes[:] = n
        out = np.where(background, 0, 255).astype(np.uint8)
        if self.detectShadows:
            sh = self._shadow(data, n, w, var, mu, Tb, TB) & ~background
            out[sh] = self.shadowValue
        return out

    def _shadow(self, data, n, w, var, mu, Tb, TB):
        npx = data.shape[1]
        res = np.zeros(npx, bool)
        done = np.zeros(npx, bool)
        tw = np.zeros(npx, F)
        for m in range(self.K):
            act = ~done & (m < n)
            if not act.any():
                break
            num = np.zeros(npx, F)
            den = np.zeros(npx, F)
            for c in range(3):
                num = num + data[c] * mu[m, c]
                den = den + mu[m, c] * mu[m, c]
            zero = act & (den == 0)
            done |= zero
            act &= ~zero
            band = act & (num <= den) & (num >= self.tau * den)
            a = num / den
            d2a = np.zeros(npx, F)
            for c in range(3):
                dd = a * mu[m, c] - data[c]
                d2a = d2a + dd * dd
            yes = band & (d2a < Tb * var[m] * a * a)
            res |= yes
            done |= yes
            act &= ~yes
            tw = np.where(act, tw + w[m], tw)
            done |= act & (tw > TB)
        return res


class MOG2Literal(MOG2):
    """The same model pixel by pixel, line for line as bgfg_gaussmix2.cpp's loop (small images: cross-check of the vectorised form)."""

    def _process(self, pix, alphaT, alpha1, prune):
        K, TB, Tg, Tb = self.K, self.TB, self.Tg, F(self.varThreshold)
        st = self.state.reshape(K, 5, -1)
        out = np.zeros(pix.shape[0], np.uint8)
        for x in range(pix.shape[0]):
            g = [[st[k, 0, x], st[k, 1, x]] for k in range(K)]                # {weight, variance}
            mean = [[st[k, 2 + c, x] for c in range(3)] for k in range(K)]
            data = [F(v) for v in pix[x]]
            background = fits = False
            nmodes = int(self.nmodes[x])
            total = F(0)
            mode = 0
            while mode < nmodes:
                weight = F(F(alpha1 * g[mode][0]) + prune)
                swap_count = 0
                if not fits:
                    v = g[mode][1]
                    dD = [F(mean[mode][c] - data[c]) for c in range(3)]
                    dist2 = F(F(F(dD[0] * dD[0]) + F(dD[1] * dD[1])) + F(dD[2] * dD[2]))
                    if total < TB and dist2 < F(Tb * v):
                        background = True
                    if dist2 < F(Tg * v):
                        fits = True
                        weight = F(weight + alphaT)
                        k = F(alphaT / weight)
                        for c in range(3):
                            mean[mode][c] = F(mean[mode][c] - F(k * dD[c]))
                        varnew = F(v + F(k * F(dist2 - v)))
                        varnew = self.varMin if varnew < self.varMin else varnew        # MAX(varnew, varMin)
                        varnew = self.varMax if varnew > self.varMax else varnew        # MIN(varnew, varMax)
                        g[mode][1] = varnew
                        for i in range(mode, 0, -1):
                            if weight < g[i - 1][0]:
                                break
                            swap_count += 1
                            g[i], g[i - 1] = g[i - 1], g[i]
                            mean[i], mean[i - 1] = mean[i - 1], mean[i]
                if weight < -prune:
                    weight = F(0)
                    nmodes -= 1
                g[mode - swap_count][0] = weight
                total = F(total + weight)
                mode += 1
            inv = F(F(1) / total) if abs(total) > EPS else F(0)
            for m in range(nmodes):
                g[m][0] = F(g[m][0] * inv)
            if not fits and alphaT > 0:
                if nmodes == K:
                    m = K - 1
                else:
                    m = nmodes
                    nmodes += 1
                if nmodes == 1:
                    g[m][0] = F(1)
                else:
                    g[m][0] = alphaT
                    for i in range(nmodes - 1):
                        g[i][0] = F(g[i][0] * alpha1)
                mean[m] = list(data)
                g[m][1] = self.varInit
                for i in range(nmodes - 1, 0, -1):
                    if alphaT < g[i - 1][0]:
                        break
                    g[i], g[i - 1] = g[i - 1], g[i]
                    mean[i], mean[i - 1] = mean[i - 1], mean[i]
            self.nmodes[x] = nmodes
            for k in range(K):
                st[k, 0, x], st[k, 1, x] = g[k]
                st[k, 2:5, x] = mean[k]
            if background:
                out[x] = 0
            elif self.detectShadows and self._shadow_px(data, nmodes, g, mean, Tb, TB):
                out[x] = self.shadowValue
            else:
                out[x] = 255
        return out

    def _shadow_px(self, data, nmodes, g, mean, Tb, TB):
        tWeight = F(0)
        for mode in range(nmodes):
            numerator = F(0)
            denominator = F(0)
            for c in range(3):
                numerator = F(numerator + F(data[c] * mean[mode][c]))
                denominator = F(denominator + F(mean[mode][c] * mean[mode][c]))
            if denominator == 0:
                return False
            if numerator <= denominator and numerator >= F(self.tau * denominator):
                a = F(numerator / denominator)
                dist2a = F(0)
                for c in range(3):
                    dD = F(F(a * mean[mode][c]) - data[c])
                    dist2a = F(dist2a + F(dD * dD))
                if dist2a < F(F(F(Tb * g[mode][1]) * a) * a):
                    return True
            tWeight = F(tWeight + g[mode][0])
            if tWeight > TB:
                return False
        return False
