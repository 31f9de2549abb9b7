// Z_FULL_FLUSH points through the JavaScript host path (streams-api.mjs -> zsnapi.node ->
// zs_pool_deflate_batch_flush): compressBatch*(inputs, format, {level, flushAt | flushEvery}),
// goldens of tests/golden/deflate_flush.json (C zlib 1.2.11), the outputs read back through
// node's own zlib -- from behind a marker too -- and the rejection rules.
//   node deflate-flush.test.mjs cpu   -- the argument checks only (no GPU needed)
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
  // not built together with the other features: refused before any device is touched
  for (const flush of [{ flushAt: [1] }, { flushEvery: 2 }]) {
    await rejects(api.compressBatch(one, "deflate-raw", { ...flush, dictionary: dict }), type, "with a dictionary: a TypeError");
    await rejects(api.compressBatch(one, "deflate", { ...flush, strategy: api.Z_FIXED }), type, "with a strategy: a TypeError");
    await rejects(api.compressBatch(one, "deflate", { ...flush, windowBits: 12 }), type, "with windowBits: a TypeError");
    await rejects(api.compressBatchSettled(one, "deflate", { ...flush, memLevel: 4 }), type, "with memLevel: a TypeError");
    await rejects(api.compressBatchDetailed(one, "deflate", { ...flush, dictionary: [dict] }), type, "the detailed entry checks it too");
  }
  for (const options of [{ flushAt: [1], flushEvery: 2 }, { flushEvery: 0 }, { flushEvery: 1.5 }, { flushEvery: -4 },
                         { flushAt: 3 }, { flushAt: [[1], [2]] }, { flushAt: [1.5] }, { flushAt: [-1] }, { flushAt: [["1"]] },
                         { flushAt: [2 ** 32] }])
    await rejects(api.compressBatch(one, "deflate", options), type, JSON.stringify(options) + ": a TypeError");
  expect(api.deflateBound(1000, "gzip", 3) === api.deflateBound(1000, "gzip") + 36, "deflateBound: 12 bytes per flush point");
}

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const golden = JSON.parse(fs.readFileSync(new URL("../../../tests/golden/deflate_flush.json", import.meta.url)));
  const text = (k, n) => corpus.text(corpus.streamSeed(k), n);
  const abc = new Uint8Array([97, 98, 99]);
  const acc = [];
  for (let k = 1, s = 0; k <= 40; k++) acc.push(s += k);
  const every = (n, step) => { const out = []; for (let p = step; p < n; p += step) out.push(p); return out; };
  // [golden, input, format, level, flushAt] -- the inputs of tests/flushcases.py
  const cases = [
    ["tiny/gzip/l6/abc@03", abc, "gzip", 6, [0, 3]],
    ["tiny/deflate/l1/abc@12", abc, "deflate", 1, [1, 2]],
    ["tiny/deflate-raw/l6/empty@0", new Uint8Array(0), "deflate-raw", 6, [0]],
    ["seams/deflate/l6/T1to40", text(6000, 820), "deflate", 6, acc],
    ["seams/deflate-raw/l1/T300x1", text(6001, 300), "deflate-raw", 1, every(300, 1)],
    ["windows/deflate-raw/l6/T200000at70000", text(6200, 200000), "deflate-raw", 6, [70000]],
    ["windows/gzip/l6/T200000at70000", text(6200, 200000), "gzip", 6, [70000]],
    ["windows/deflate-raw/l9/T200000every65536", text(6200, 200000), "deflate-raw", 9, every(200000, 65536)],
  ];
  const inflate = { "deflate-raw": zlib.inflateRawSync, deflate: zlib.inflateSync, gzip: zlib.gunzipSync };
  for (const [name, x, format, level, flushAt] of cases) {
    expect(golden[name] !== undefined, "golden " + name);
    const want = JSON.stringify(golden[name].slice(0, 2));
    const options = { level, flushAt: [flushAt, null, flushAt] };
    const inputs = [x, x, x];
    const outs = await api.compressBatch(inputs, format, options);
    expect(JSON.stringify(digest(outs[0])) === want, name + ": zlib 1.2.11's bytes");
    expect(same(outs[0], outs[2]), name + ": the same input twice");
    expect(same(outs[1], (await api.compressBatch([x], format, { level }))[0]), name + ": no flush point is the plain stream");
    outs.forEach((o, i) => expect(same(new Uint8Array(inflate[format](o)), x), `${name}: node's zlib, input ${i}`));
    if (format === "deflate-raw")  // a decoder restarts behind every marker
      golden[name][2].forEach((off, k) => expect(same(new Uint8Array(zlib.inflateRawSync(outs[0].subarray(off))), x.subarray(flushAt[k])),
                                                 `${name}: restart at ${off}`));
    const back = await api.decompressBatch(outs, format);
    back.forEach((o, i) => expect(same(o, x), `${name}: the engine's inflate, input ${i}`));
    expect(same((await api.compressBatch([x], format, { level, flushAt }))[0], outs[0]), name + ": one list for every input");
    const det = await api.compressBatchDetailed(inputs, format, options);
    det.outputs.forEach((o, i) => expect(det.status[i] === 1 && same(o, outs[i]), `${name}: detailed, input ${i}`));
    expect(format === "deflate-raw" ? det.check[0] === 1 : det.check[0] === det.check[1], name + ": the check value covers the whole stream");
    const settled = await api.compressBatchSettled(inputs, format, options);
    settled.forEach((s, i) => expect(s.status === "fulfilled" && same(s.value, outs[i]), `${name}: settled, input ${i}`));
  }
  // flushEvery is flushAt at N, 2N, ...
  const x = text(6200, 200000);
  const a = await api.compressBatch([x, x.subarray(0, 65536)], "deflate-raw", { level: 9, flushEvery: 65536 });
  expect(JSON.stringify(digest(a[0])) === JSON.stringify(golden["windows/deflate-raw/l9/T200000every65536"].slice(0, 2)), "flushEvery");
  expect(same(a[1], (await api.compressBatch([x.subarray(0, 65536)], "deflate-raw", { level: 9 }))[0]), "flushEvery: none below the length");
  // the entry's refusals: "init failed: -2", code "-2" from the detailed entry
  for (const flushAt of [[5, 4], [3, 3], [200001]]) {
    await rejects(api.compressBatch([x], "deflate", { level: 6, flushAt }), (e) => e.message === "init failed: -2", "positions " + flushAt);
    await rejects(api.compressBatchDetailed([x], "deflate", { level: 6, flushAt }), (e) => e.code === "-2", "detailed: positions " + flushAt);
  }
  await rejects(api.compressBatch([x], "deflate", { level: 0, flushAt: [5] }), (e) => e.message === "init failed: -2", "level 0");
  await rejects(api.compressBatch([x], "deflate", { level: 10, flushAt: [5] }), (e) => e.message === "init failed: -2", "level 10");
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e); process.exit(1); });
