------------------------------ MODULE ring_strong ------------------------------
(* Written to show: THE KERNELS AT SIZE (specs_liveprops/ring_cut.tla's shape).  A fair counter cycles modulo N until a strongly fair process stops it, which it can do at c = Half - 1 only.  The ring is one component of N states, blocked by the stopper; the first round closes the one state that enables it.  What is left is a path of N - 1 states: the second round's component build is all trimming, one-state components in which the counter is enabled and never taken, every one of them closed.  Termination and <>(stop = 1) HOLD after two rounds; under weak fairness of the stopper both are violated. *)
EXTENDS Naturals
CONSTANTS N, Half
(* --algorithm ring_strong
variables c = 0, stop = 0;

fair process Counter = 0
begin
  C: while stop = 0 do
       c := (c + 1) % N;
     end while;
end process

fair+ process Stopper = 1
begin
  S: await c = Half - 1;
     stop := 1;
end process

end algorithm *)

Stops == <>(stop = 1)
=============================================================================
