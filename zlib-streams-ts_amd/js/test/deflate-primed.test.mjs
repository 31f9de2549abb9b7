// Primed pieces through the JavaScript host path (streams-api.mjs -> zsnapi.node ->
// zs_pool_deflate_batch_primed): compressBatch*(inputs, format, {level, flushAt | flushEvery, primed: true}),
// goldens of tests/golden/deflate_primed.json (C zlib 1.2.11), the outputs read back as ONE stream through
// node's own zlib and the engine's inflate, and the rejection rules.
//   node deflate-primed.test.mjs cpu   -- the argument checks only (no GPU needed)
import crypto from "crypto";
import fs from "fs";
import zlib from "zlib";

import * as corpus from "../../../tests/golden/corpus.mjs";
import * as api from "../streams-api.mjs";

let checks = 0;
const expect = (c, m) => { if (!c) throw new Error("FAIL " + m); checks++; };
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) === 0;
const digest = (b) => [b.length, crypto.createHash("sha256").update(b).digest("hex").slice(0, 16)];

async function rejects(p, pred, what) {
  let e = null;
  try { await p; } catch (x) { e = x; }
  expect(e !== null && pred(e), what + (e ? ": " + e.message : ": no error"));
}

async function argumentChecks() {
  const one = [new Uint8Array([1, 2, 3])];
  const dict = new Uint8Array([1, 2, 3, 4]);
  const type = (e) => e instanceof TypeError;
  // without positions it is an error; not built together with the other features: refused before any device is touched
  await rejects(api.compressBatch(one, "deflate", { primed: true }), type, "primed without positions: a TypeError");
  await rejects(api.compressBatchDetailed(one, "deflate", { primed: true }), type, "the detailed entry checks it too");
  await rejects(api.compressBatchSettled(one, "deflate", { primed: true }), type, "the settled entry checks it too");
  await rejects(api.compressBatch(one, "deflate", { primed: 1, flushAt: [1] }), type, "primed: 1 is a TypeError");
  for (const flush of [{ flushAt: [1] }, { flushEvery: 2 }]) {
    const o = { ...flush, primed: true };
    await rejects(api.compressBatch(one, "deflate-raw", { ...o, dictionary: dict }), type, "with a dictionary: a TypeError");
    await rejects(api.compressBatch(one, "deflate", { ...o, strategy: api.Z_FIXED }), type, "with a strategy: a TypeError");
    await rejects(api.compressBatch(one, "deflate", { ...o, windowBits: 12 }), type, "with windowBits: a TypeError");
    await rejects(api.compressBatchSettled(one, "deflate", { ...o, memLevel: 4 }), type, "with memLevel: a TypeError");
    await rejects(api.compressBatch(one, "gzip", { ...o, bgzf: true }), type, "with bgzf: a TypeError");
    await rejects(api.compressBatchDetailed(one, "deflate", { ...o, dictionary: [dict] }), type, "the detailed entry checks it too");
  }
  await rejects(api.compressBatch(one, "deflate", { primed: true, flushAt: [1], flushEvery: 2 }), type, "flushAt and flushEvery");
  expect(api.deflateBound(1000, "gzip", 3) === api.deflateBound(1000, "gzip") + 36, "deflateBound: 12 bytes per point");
}

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const golden = JSON.parse(fs.readFileSync(new URL("../../../tests/golden/deflate_primed.json", import.meta.url)));
  const text = (k, n) => corpus.text(corpus.streamSeed(k), n);
  const abc = new Uint8Array([97, 98, 99]);
  const acc = [];
  for (let k = 1, s = 0; k <= 40; k++) acc.push(s += k);
  const every = (n, step) => { const out = []; for (let p = step; p < n; p += step) out.push(p); return out; };
  // [golden, input, format, level, flushAt] -- the inputs of tests/primedcases.py
  const cases = [
    ["tiny/gzip/l6/abc@03", abc, "gzip", 6, [0, 3]],
    ["tiny/deflate/l1/abc@12", abc, "deflate", 1, [1, 2]],
    ["tiny/deflate-raw/l6/empty@0", new Uint8Array(0), "deflate-raw", 6, [0]],
    ["seams/deflate/l6/T1to40", text(6000, 820), "deflate", 6, acc],
    ["seams/deflate-raw/l1/T300x1", text(6001, 300), "deflate-raw", 1, every(300, 1)],
    ["prime/deflate-raw/l6/T70000at32768", text(7000, 70000), "deflate-raw", 6, [32768]],
    ["prime/deflate-raw/l3/T70000at2", text(7000, 70000), "deflate-raw", 3, [2]],
    ["windows/deflate-raw/l9/T32768+32770", text(7200, 32768 + 32770), "deflate-raw", 9, [32768]],
    ["long/deflate-raw/l6/T400000_0", text(7700, 400000), "deflate-raw", 6, every(400000, 131072)],
  ];
  const inflate = { "deflate-raw": zlib.inflateRawSync, deflate: zlib.inflateSync, gzip: zlib.gunzipSync };
  for (const [name, x, format, level, flushAt] of cases) {
    expect(golden[name] !== undefined, "golden " + name);
    const want = JSON.stringify(golden[name].slice(0, 2));
    const options = { level, primed: true, flushAt: [flushAt, null, flushAt] };
    const inputs = [x, x, x];
    const outs = await api.compressBatch(inputs, format, options);
    expect(JSON.stringify(digest(outs[0])) === want, name + ": zlib 1.2.11's bytes");
    expect(same(outs[0], outs[2]), name + ": the same input twice");
    expect(same(outs[1], (await api.compressBatch([x], format, { level }))[0]), name + ": no point is the plain stream");
    outs.forEach((o, i) => expect(same(new Uint8Array(inflate[format](o)), x), `${name}: node's zlib reads one stream, input ${i}`));
    if (format === "deflate-raw")  // every piece but the last ends with the marker on a byte boundary
      golden[name][2].forEach((off) => expect(outs[0][off - 4] === 0 && outs[0][off - 3] === 0 && outs[0][off - 2] === 255 && outs[0][off - 1] === 255,
                                              `${name}: the marker before ${off}`));
    const back = await api.decompressBatch(outs, format);
    back.forEach((o, i) => expect(same(o, x), `${name}: the engine's inflate, input ${i}`));
    expect(same((await api.compressBatch([x], format, { level, primed: true, flushAt }))[0], outs[0]), name + ": one list for every input");
    const det = await api.compressBatchDetailed(inputs, format, options);
    det.outputs.forEach((o, i) => expect(det.status[i] === 1 && same(o, outs[i]), `${name}: detailed, input ${i}`));
    expect(format === "deflate-raw" ? det.check[0] === 1 : det.check[0] === det.check[1], name + ": the check value covers the whole stream");
    const settled = await api.compressBatchSettled(inputs, format, options);
    settled.forEach((s, i) => expect(s.status === "fulfilled" && same(s.value, outs[i]), `${name}: settled, input ${i}`));
    const flushed = (await api.compressBatch([x], format, { level, flushAt }))[0];
    if (x.length > 60000) expect(outs[0].length < flushed.length, name + ": smaller than flushed at the same positions");
  }
  // flushEvery is flushAt at N, 2N, ...
  const x = text(7700, 400000);
  const a = await api.compressBatch([x, x.subarray(0, 131072)], "deflate-raw", { level: 6, primed: true, flushEvery: 131072 });
  expect(JSON.stringify(digest(a[0])) === JSON.stringify(golden["long/deflate-raw/l6/T400000_0"].slice(0, 2)), "flushEvery");
  expect(same(a[1], (await api.compressBatch([x.subarray(0, 131072)], "deflate-raw", { level: 6 }))[0]), "flushEvery: none below the length");
  // the entry's refusals: "init failed: -2", code "-2" from the detailed entry
  for (const flushAt of [[5, 4], [3, 3], [400001]]) {
    await rejects(api.compressBatch([x], "deflate", { level: 6, primed: true, flushAt }), (e) => e.message === "init failed: -2", "positions " + flushAt);
    await rejects(api.compressBatchDetailed([x], "deflate", { level: 6, primed: true, flushAt }), (e) => e.code === "-2", "detailed: positions " + flushAt);
  }
  await rejects(api.compressBatch([x], "deflate", { level: 0, primed: true, flushAt: [5] }), (e) => e.message === "init failed: -2", "level 0");
  await rejects(api.compressBatch([x], "deflate", { level: 10, primed: true, flushAt: [5] }), (e) => e.message === "init failed: -2", "level 10");
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e); process.exit(1); });
